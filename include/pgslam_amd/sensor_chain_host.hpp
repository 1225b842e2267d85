// sensor_chain_host.hpp -- the per-point statements of the sensor filter chain (include/pgicp_sensor_chain.h) in plain C++: the
// observation direction, OrientNormals' flip test, Shadow's keep test and SimpleSensorNoise's value.  The device kernels
// (pgslam_amd/csrc/k_sensor_chain.inc), the C++ drop-in's host filters (pointmatcher.hpp) and the stand-alone test program
// (tests/cpp/test_sensor_chain_cpu.cpp) all call these functions, so the three cannot drift apart.  Everything is in T; no product
// is fused with a sum (the translation units that include this are built without contraction); the root is the correctly
// rounded one and divisions are IEEE.
#pragma once

#include <cmath>

#ifndef PGSLAM_CHAIN_HD
#define PGSLAM_CHAIN_HD         // (the device library defines it as __host__ __device__ before it includes this)
#endif

namespace pgslam_amd {
namespace sensor_chain {

PGSLAM_CHAIN_HD inline float sqrt_rn(float v) { return __builtin_sqrtf(v); }
PGSLAM_CHAIN_HD inline double sqrt_rn(double v) { return __builtin_sqrt(v); }

// ObservationDirection: obs[a] = c[a] - x[a]
template <typename T>
PGSLAM_CHAIN_HD inline void observation_direction(const T c[3], const T x[3], T obs[3])
{
    for (int a = 0; a < 3; a++) obs[a] = c[a] - x[a];
}

// OrientNormals: dot = ((0 + n0 o0) + n1 o1) + n2 o2; the normal is negated when towardCenter ? dot < 0 : dot > 0
template <typename T>
PGSLAM_CHAIN_HD inline bool orient_flips(const T n[3], const T o[3], bool toward_center)
{
    T dot = 0;
    for (int a = 0; a < 3; a++) dot += n[a] * o[a];
    return toward_center ? dot < 0 : dot > 0;
}

// v / |v| when the squared norm (x x + y y) + z z is > 0; v as it is otherwise
template <typename T>
PGSLAM_CHAIN_HD inline void normalized(T &x, T &y, T &z)
{
    const T zz = (x * x + y * y) + z * z;
    if (zz > T(0)) { const T s = sqrt_rn(zz); x = x / s; y = y / s; z = z / s; }
}

// Shadow's threshold from the angle: sin(eps) in T with the C library, on the host
template <typename T>
inline T shadow_threshold(T eps_angle) { return std::sin(eps_angle); }
inline bool shadow_eps_ok(double e) { return e >= 0.0 && e <= 3.14159265358979323846; }

// Shadow (orc_shadow_keep): the point stays while |normal.normalized() . position.normalized()| > sin_eps
template <typename T>
PGSLAM_CHAIN_HD inline bool shadow_keep(const T n[3], const T x[3], T sin_eps)
{
    T ax = n[0], ay = n[1], az = n[2], bx = x[0], by = x[1], bz = x[2];
    normalized(ax, ay, az);
    normalized(bx, by, bz);
    const T d = (ax * bx + ay * by) + az * bz;
    return (d < T(0) ? -d : d) > sin_eps;
}

// SimpleSensorNoise: (minRadius, beamAngle, beamConst) of a sensorType, each rounded to T; false: no such type
template <typename T>
struct NoiseModel { int sensor_type = 0; T min_r = 0, angle = 0, cst = 0, gain = 0; };
template <typename T>
inline bool noise_model(int sensor_type, T gain, NoiseModel<T> &m)
{
    static const double prm[5][3] = {{0.012, 0.0068, 0.0008}, {0.028, 0.0013, 0.0001}, {0.018, 0.0006, 0.0015}, {0, 0, 0}, {0.004, 0.0053, -0.0092}};
    if (sensor_type < 0 || sensor_type > 4) return false;
    m.sensor_type = sensor_type;
    m.min_r = (T)prm[sensor_type][0]; m.angle = (T)prm[sensor_type][1]; m.cst = (T)prm[sensor_type][2];
    m.gain = gain;
    return true;
}
// orc_simple_sensor_noise: r = sqrt((x x + y y) + z z); type 3: (r r) T(0.5 * 0.00285), else max(minRadius, beamAngle r + beamConst); times gain
template <typename T>
PGSLAM_CHAIN_HD inline T noise_value(const NoiseModel<T> &m, const T x[3])
{
    const T r = sqrt_rn((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    T v;
    if (m.sensor_type == 3) v = (r * r) * (T)(0.5 * 0.00285);
    else { v = m.angle * r + m.cst; if (v < m.min_r) v = m.min_r; }
    return m.gain * v;
}

}  // namespace sensor_chain
}  // namespace pgslam_amd
