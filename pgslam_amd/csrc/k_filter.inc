// k_filter.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): the localizer's input filters
// on the device.
//
// pgslam applies a YAML list of DataPointsFilters to every scan IN PLACE and then moves it from the sensor's frame into the
// robot's (input_filters_.apply at /root/reference/src/pgslam/Localizer.hpp:103, rigid_transformation_->compute at :106).  The
// filters that only drop points -- BoundingBox, MinDist, MaxDist, RemoveNaN, FixStepSampling, (seeded) RandomSampling -- are
// predicates of a point's own coordinates or of its index in the cloud the filter is handed; here the list runs as flag
// passes over the uploaded scan, one exclusive scan wherever a filter needs the points' current indices, and ONE compaction
// that also applies the sensor transform: what comes out is the filtered, transformed cloud, on the device for the ICP and on
// its way back to the caller's host cloud.  The kept points are those libpointmatcher's filters keep ([EXT] DataPointsFilters/
// MaxDist.cpp, MinDist.cpp, BoundingBox.cpp, RemoveNaN.cpp, restated in oracle/icp_oracle.c: orc_filter_chain) and those the host
// filters of include/pgslam_amd/pointmatcher.hpp keep, index for index (tests compare all three): the same predicates in the same
// arithmetic -- a radius is the norm of the point in T, sqrt((x x + y y) + z z) correctly rounded, compared strictly.
struct FilterDev { int type; int pad_; double p[8]; };

#define PGICP_F_IDENTITY 0
#define PGICP_F_MAX_DIST 1
#define PGICP_F_MIN_DIST 2
#define PGICP_F_BOUNDING_BOX 3
#define PGICP_F_REMOVE_NAN 4
#define PGICP_F_FIX_STEP 5
#define PGICP_F_RANDOM_SAMPLING 6
#define PGICP_F_MAX_POINT_COUNT 7
#define PGICP_F_MAX_QUANTILE_ON_AXIS 8       // (include/pgicp_quantile.h; its kernels: k_axisquantile.inc)
#define PGICP_F_CUT_AT_DESCRIPTOR 9          // (include/pgicp_descriptor_filters.h; the test: descriptor_filters_host.hpp's cut_keep)

__device__ __forceinline__ float sqrt_rn(float v) { return __builtin_sqrtf(v); }      // (correctly rounded; __fsqrt_rn is the native 1-ulp one)
__device__ __forceinline__ double sqrt_rn(double v) { return __builtin_sqrt(v); }

struct FilterList { int n; int pad_; FilterDev f[8]; };

// filters [first, last) of the list, all of them point-wise: a point's flag goes to 0 when one of them drops it (desc, drows: the
// descriptors a CutAtDescriptor entry reads; the list's check has made sure they are there and hold its row)
template <typename T>
__global__ __launch_bounds__(256) void k_filter_points(const T *__restrict__ feat, int fstride, int frows, const T *__restrict__ desc,
                                                        int drows, int n, FilterList fl, int first, int last, int *__restrict__ keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const T *q = feat + (long long)i * fstride;
    const T x = q[0], y = q[1], z = q[2];
    bool ok = true;
    for (int k = first; k < last && ok; ++k) {
        const FilterDev &f = fl.f[k];
        if (f.type == PGICP_F_MAX_DIST || f.type == PGICP_F_MIN_DIST) {
            // [EXT] MaxDist.cpp / MinDist.cpp: dim = -1: norm < |maxDist| (norm > |minDist|); else features(dim) < maxDist (> minDist);
            // p[1] = dim + 1, so that the zero of an older caller means the radius.  A NaN fails both comparisons: dropped.
            const int dim = (int)f.p[1] - 1;
            const T lim = (T)f.p[0];                                // (the limit arrives rounded to T, as the host filter holds it)
            if (dim < 0) {
                const T r = sqrt_rn((x * x + y * y) + z * z), al = lim < (T)0 ? -lim : lim;
                ok = f.type == PGICP_F_MAX_DIST ? r < al : r > al;
            } else {
                const T v = q[dim];
                ok = f.type == PGICP_F_MAX_DIST ? v < lim : v > lim;
            }
        } else if (f.type == PGICP_F_BOUNDING_BOX) {
            const bool in = (T)f.p[0] < x && x < (T)f.p[3] && (T)f.p[1] < y && y < (T)f.p[4] && (T)f.p[2] < z && z < (T)f.p[5];
            ok = in != (f.p[6] != 0.0);
        } else if (f.type == PGICP_F_REMOVE_NAN) {
            for (int r = 0; r < frows; ++r) ok = ok && q[r] == q[r];
        } else if (f.type == PGICP_F_CUT_AT_DESCRIPTOR) {
            // p[0] = the row, p[1] = useLargerThan, p[2] = the threshold (it arrives rounded to T)
            ok = pgslam_amd::descriptor_filters::cut_keep<T>(desc[(long long)i * drows + (int)f.p[0]], (T)f.p[2], f.p[1] != 0.0);
        }
    }
    if (!ok) keep[i] = 0;
}

__device__ __forceinline__ unsigned long long splitmix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ULL; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// the hash behind every seeded draw: element i of seed's stream.  The caller takes its bits (>> 11 for a double in [0, 1), ...)
__device__ __forceinline__ unsigned long long seeded_mix(unsigned long long seed, unsigned long long i) { return splitmix(seed * 0x100000001B3ULL + i); }

// one index-dependent filter: `rank` = the point's index in the cloud this filter is handed (exclusive scan of the flags)
__global__ __launch_bounds__(256) void k_filter_index(int n, FilterDev f, const int *__restrict__ rank, int *__restrict__ keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int j = rank[i];
    bool ok = true;
    if (f.type == PGICP_F_FIX_STEP) ok = j % (int)f.p[0] == 0;
    else if (f.type == PGICP_F_RANDOM_SAMPLING)
        ok = (double)(seeded_mix((unsigned long long)f.p[1], j) >> 11) / 9007199254740992.0 < f.p[0];
    else if (f.type == PGICP_F_MAX_POINT_COUNT) {
        // [EXT] MaxPointCount.cpp (the vintage pgslam was written against): only when maxCount < N, a random sample with
        // prob = T(maxCount) / T(N); N = the points this filter is handed = rank[n]; prob_bits: that quotient, made by the host in T
        const int total = rank[n];
        if ((double)total > f.p[0])
            ok = (double)(seeded_mix((unsigned long long)f.p[1], j) >> 11) / 9007199254740992.0 <
                 (f.p[2] != 0.0 ? (double)((float)f.p[0] / (float)total) : f.p[0] / (double)total);
    }
    if (!ok) keep[i] = 0;
}

// compaction + RigidTransformation::compute: features' = T features (rows 0..2; the other rows are copied), the descriptor
// rows [rot0, rot0 + 3) and [rot1, rot1 + 3) (normals, observationDirections; -1: none) are rotated, the rest copied
template <typename T>
__global__ __launch_bounds__(256) void k_filter_compact(const T *__restrict__ feat, int fstride, int frows, const T *__restrict__ desc,
                                                         int drows, int n, const int *__restrict__ keep, const int *__restrict__ pos,
                                                         Mat34 M, int transform, int rot0, int rot1, T *__restrict__ out_feat,
                                                         T *__restrict__ out_desc, int *__restrict__ kept_idx, int *__restrict__ dropped,
                                                         int dropped_cap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!keep[i]) {
        // the dropped points' indices, ascending without a sort: i - pos[i] points were dropped before point i
        if (dropped) { const int d = i - pos[i]; if (d < dropped_cap) dropped[d] = i; }
        return;
    }
    const long long o = pos[i];
    const T *q = feat + (long long)i * fstride;
    T *of = out_feat + o * fstride;
    const T r00 = (T)M.v[0], r01 = (T)M.v[1], r02 = (T)M.v[2], r10 = (T)M.v[4], r11 = (T)M.v[5], r12 = (T)M.v[6],
            r20 = (T)M.v[8], r21 = (T)M.v[9], r22 = (T)M.v[10];
    if (transform) {
        const T x = q[0], y = q[1], z = q[2];
        of[0] = ((r00 * x + r01 * y) + r02 * z) + (T)M.v[3];
        of[1] = ((r10 * x + r11 * y) + r12 * z) + (T)M.v[7];
        of[2] = ((r20 * x + r21 * y) + r22 * z) + (T)M.v[11];
    } else { of[0] = q[0]; of[1] = q[1]; of[2] = q[2]; }
    for (int r = 3; r < frows; ++r) of[r] = q[r];
    if (desc) {
        const T *d = desc + (long long)i * drows;
        T *od = out_desc + o * drows;
        for (int r = 0; r < drows; ++r) od[r] = d[r];
        if (transform) {
            for (int g = 0; g < 2; ++g) {
                const int r0 = g == 0 ? rot0 : rot1;
                if (r0 < 0) continue;
                const T x = d[r0], y = d[r0 + 1], z = d[r0 + 2];
                od[r0] = (r00 * x + r01 * y) + r02 * z;
                od[r0 + 1] = (r10 * x + r11 * y) + r12 * z;
                od[r0 + 2] = (r20 * x + r21 * y) + r22 * z;
            }
        }
    }
    if (kept_idx) kept_idx[o] = i;
}

__global__ __launch_bounds__(256) void k_fill_int(int *__restrict__ a, int n, int v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}
