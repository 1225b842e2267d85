// api_noise.inc -- part of pgicp_api.cpp (one translation unit): include/pgicp_noise.h -- the SimpleSensorNoise descriptor, arming an
// ICP call with its readings' noise rows, and the armed call's reduction over its last error elements.

// An armed noise is consumed by the ICP call that finds it, whatever becomes of that call: returns whether there was one.  The
// previous armed call's results are void from here on.
static bool noise_take(pgicp_ctx *c)
{
    if (!c) return false;
    const bool armed = c->noise.armed;
    c->noise.armed = false;
    c->noise.last_P = -1;
    return armed;
}

template <typename T>
int simple_sensor_noise(pgicp_ctx *c, const T *xyz, int stride, int n, int mem, int sensor_type, double gain, T *out, int out_mem)
{
    if (!c || n < 0 || (n > 0 && (!xyz || !out)) || stride < 3 || (mem != PGICP_HOST && mem != PGICP_DEVICE) ||
        (out_mem != PGICP_HOST && out_mem != PGICP_DEVICE))
        return fail(c, PGICP_ERR_ARG, "pgicp_simple_sensor_noise: bad argument");
    // (minRadius, beamAngle, beamConst) per sensorType, each rounded to T as the filter holds them
    T min_r = 0, angle = 0, cst = 0;
    switch (sensor_type) {
    case 0: min_r = (T)0.012; angle = (T)0.0068; cst = (T)0.0008; break;
    case 1: min_r = (T)0.028; angle = (T)0.0013; cst = (T)0.0001; break;
    case 2: min_r = (T)0.018; angle = (T)0.0006; cst = (T)0.0015; break;
    case 3: break;
    case 4: min_r = (T)0.004; angle = (T)0.0053; cst = (T)-0.0092; break;
    default: return fail(c, PGICP_ERR_ARG, "SimpleSensorNoiseDataPointsFilter: sensorType must be 0 .. 4, got " + std::to_string(sensor_type));
    }
    if (n == 0) return PGICP_OK;
    HIPC(c, hipSetDevice(c->device));
    UploadUse uu(c);
    State<T> &S = state<T>(c);
    const T *d_xyz = nullptr;
    if (mem == PGICP_HOST) HIPC(c, S.staging.ensure(staged_bytes(sizeof(T), stride, n)));
    { const int st = to_device<T>(c, xyz, stride, n, mem, S.staging, 0, &d_xyz); if (st) return st; }
    T *d_out = out;
    if (out_mem == PGICP_HOST) { HIPC(c, S.stage_aux.ensure(sizeof(T) * (size_t)n)); d_out = S.stage_aux.template as<T>(); }
    launch_simple_sensor_noise<T>(c->stream, d_xyz, stride, n, sensor_type, min_r, angle, cst, (T)gain, d_out);
    if (out_mem == PGICP_HOST) XFER(c, d2h(c, out, d_out, sizeof(T) * (size_t)n));
    HIPC(c, stream_sync(c));
    HIPC(c, hipGetLastError());
    return PGICP_OK;
}

// One value per reading point of every problem, copied into the context for the next call to consume: the noise rows here, and
// KDTreeVarDistMatcher's radii (api_vardist.inc).  `what`: the entry point's name for the messages; `inf_ok`: +inf is a value (a
// radius that cuts nothing) -- otherwise a value must be finite; neither takes a negative value or a NaN.  `stage`: the kernel that
// copies a device row and raises the flag at a refused value.
template <typename T>
int arm_rows(pgicp_ctx *c, pgicp_ctx::ArmedRows &N, const char *what, bool inf_ok, void (*stage)(hipStream_t, const T *, int, int, T *, int *),
             int P, const T *const *rows, const int *stride, const int *n, int mem)
{
    N.armed = false;
    if (P <= 0 || P > 65535 || !rows || !stride || !n || (mem != PGICP_HOST && mem != PGICP_DEVICE))
        return fail(c, PGICP_ERR_ARG, std::string(what) + ": bad argument");
    size_t total = 0;
    for (int p = 0; p < P; p++) {
        if (!rows[p]) continue;
        if (stride[p] < 1 || n[p] <= 0) return fail(c, PGICP_ERR_ARG, std::string(what) + ": bad stride or size of problem " + std::to_string(p));
        total += (size_t)n[p];
    }
    HIPC(c, hipSetDevice(c->device));
    N.off.assign(P, -1);
    N.n.assign(P, 0);
    N.bad = false;
    N.elem = (int)sizeof(T);
    // the offsets, then one int: the staging kernel's flag
    const size_t flag_off = sizeof(long long) * (size_t)P;
    HIPC(c, N.off_dev.ensure(flag_off + sizeof(int)));
    HIPC(c, N.vals.ensure(sizeof(T) * std::max<size_t>(total, 1)));
    long long off = 0;
    for (int p = 0; p < P; p++) if (rows[p]) { N.off[p] = off; N.n[p] = n[p]; off += n[p]; }
    XFER(c, h2d(c, N.off_dev.p, N.off.data(), flag_off));
    if (mem == PGICP_HOST) {
        // packed and looked at on the host, one copy for the batch
        std::vector<T> packed(total);
        size_t k = 0;
        for (int p = 0; p < P; p++) {
            if (!rows[p]) continue;
            for (int i = 0; i < n[p]; i++) {
                const T v = rows[p][(size_t)i * stride[p]];
                if (!(v >= (T)0) || (!inf_ok && !std::isfinite(v))) N.bad = true;
                packed[k++] = v;
            }
        }
        XFER(c, h2d(c, N.vals.p, packed.data(), sizeof(T) * total));
        HIPC(c, stream_sync(c));
    } else {
        UploadUse uu(c);
        int *flag = (int *)((char *)N.off_dev.p + flag_off);
        HIPC(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        for (int p = 0; p < P; p++) {
            if (!rows[p]) continue;
            uu.touch(rows[p]);
            stage(c->stream, rows[p], stride[p], n[p], N.vals.template as<T>() + N.off[p], flag);
        }
        int bad = 0;
        XFER(c, d2h(c, &bad, flag, sizeof(int)));
        HIPC(c, stream_sync(c));
        HIPC(c, hipGetLastError());
        N.bad = bad != 0;
    }
    N.armed = true;
    return PGICP_OK;
}
template <typename T>
int arm_reading_noise(pgicp_ctx *c, int P, const T *const *noise, const int *stride, const int *n, int mem)
{
    if (!c) return PGICP_ERR_ARG;
    return arm_rows<T>(c, c->noise, "pgicp_arm_reading_noise", false, launch_noise_stage<T>, P, noise, stride, n, mem);
}

// The consuming call's look at what was armed (before it does any work): the batch's shape and element type, the values
// (`what`: "sensor noise" / "reading radii", for the messages)
template <typename T>
int rows_check(pgicp_ctx *c, const pgicp_ctx::ArmedRows &N, const std::string &what, const char *bad, int P, const pgicp_problem *pr)
{
    if (N.elem != (int)sizeof(T)) return fail(c, PGICP_ERR_ARG, what + ": armed with another element type than the call's");
    if ((int)N.off.size() != P)
        return fail(c, PGICP_ERR_ARG, what + ": armed for " + std::to_string(N.off.size()) + " problems, the call has " + std::to_string(P));
    for (int p = 0; p < P; p++)
        if (N.off[p] >= 0 && N.n[p] != pr[p].n)
            return fail(c, PGICP_ERR_ARG, what + ": " + std::to_string(N.n[p]) + " values armed for problem " + std::to_string(p) + ", its reading has " + std::to_string(pr[p].n) + " points");
    if (N.bad) return fail(c, PGICP_ERR_ARG, what + ": " + bad);
    return PGICP_OK;
}
template <typename T>
int noise_check(pgicp_ctx *c, int P, const pgicp_problem *pr)
{
    return rows_check<T>(c, c->noise, "sensor noise", "a value is negative or not finite", P, pr);
}
