"""A numpy statement of include/pgicp_descriptor_filters.h: the three per-point statements (IncidenceAngle, Sphericality,
CutAtDescriptorThreshold) and pgicp_sensor_chain_ext_*, the latter composed from tests/sensor_chain_ref.py's pieces (head,
observation_direction, orient_flips, the oracle's shadow, density and noise functions).  The arctangent is restated here in float64
numpy, operation by operation; tests/test_descriptor_filters_host.py pins it against the oracle's orc_atan2 and the product's
det_atan2 to the bit, and pins the drop-in's host filters against this file; the library sits against it
(tests/test_gpu_descriptor_filters.py)."""
import numpy as np

import sensor_chain_ref as sc

TYPES, KNN, SIZES, MAIN_N, EPS, CENTER, SEED = sc.TYPES, sc.KNN, sc.SIZES, sc.MAIN_N, sc.EPS, sc.CENTER, sc.SEED
OBS, ORIENT, SHADOW, MAXDENS, NOISE = sc.OBS, sc.ORIENT, sc.SHADOW, sc.MAXDENS, sc.NOISE
INC, SPH, CUT = "incidence_angle", "sphericality", "cut_at_descriptor"
ALL = ("normals", "eigen_values", "densities")
ROWS = sc.ROWS + ("incidence_angles", "sphericality", "unstructureness", "structureness")
# the name a cut gives -> the key of run()'s result
CUT_ROWS = dict(densities="densities", incidence_angles="incidence_angles", sphericality="sphericality", unstructureness="unstructureness",
                structureness="structureness", simple_sensor_noise="noise")

_HI = np.array([4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00])
_LO = np.array([2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17])
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
       9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
       4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)


def atan_pos(x):
    """the published fdlibm atan for x >= 0 in float64: reduction at 7/16, 11/16, 19/16, 39/16, an odd polynomial of degree 23"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = x.copy()
        idx = np.full(x.shape, -1)
        m = (x >= 0.4375) & (x < 0.6875)
        idx[m], r[m] = 0, ((2.0 * x - 1.0) / (2.0 + x))[m]
        m = (x >= 0.6875) & (x < 1.1875)
        idx[m], r[m] = 1, ((x - 1.0) / (x + 1.0))[m]
        m = (x >= 1.1875) & (x < 2.4375)
        idx[m], r[m] = 2, ((x - 1.5) / (1.0 + 1.5 * x))[m]
        m = (x >= 2.4375) & (x < 7.378697629483821e+19)
        idx[m], r[m] = 3, (-1.0 / x)[m]
        z = r * r
        w = z * z
        s1 = z * (_AT[0] + w * (_AT[2] + w * (_AT[4] + w * (_AT[6] + w * (_AT[8] + w * _AT[10])))))
        s2 = w * (_AT[1] + w * (_AT[3] + w * (_AT[5] + w * (_AT[7] + w * _AT[9]))))
        k = np.maximum(idx, 0)
        out = np.where(idx < 0, r - r * (s1 + s2), _HI[k] - ((r * (s1 + s2) - _LO[k]) - r))
        out = np.where(x < 1.862645149230957e-09, x, out)
        out = np.where(x >= 7.378697629483821e+19, _HI[3] + _LO[3], out)
    return out


def atan2(y, x):
    """det_atan2 / orc_atan2 in float64 numpy"""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    pi, pi_lo, half_pi = 3.1415926535897931160e+00, 1.2246467991473531772e-16, 1.57079632679489655800e+00 + 6.12323399573676603587e-17
    with np.errstate(all="ignore"):
        z = atan_pos(np.abs(y / x))
        out = np.where(x > 0.0, np.where(y > 0.0, z, -z), np.where(y > 0.0, pi - (z - pi_lo), (z - pi_lo) - pi))
        out = np.where(x == 0.0, np.where(y > 0.0, half_pi, -half_pi), out)
        out = np.where(y == 0.0, np.where((x > 0.0) | ((x == 0.0) & ~np.signbit(x)), y, np.where(np.signbit(y), -pi, pi)), out)
        out = np.where(np.isnan(y) | np.isnan(x), y + x, out)
    return out


def acos(c):
    """det_acos in float64: c clamped to [-1, 1], atan2(sqrt((1 - c) (1 + c)), c); a NaN stays a NaN"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = np.where(c < -1.0, -1.0, c)
        k = np.where(k > 1.0, 1.0, k)
        return np.where(np.isnan(c), c, atan2(np.sqrt((1.0 - k) * (1.0 + k)), k))


def normalized(v, T):
    """v / |v| in T where the squared norm (x x + y y) + z z is > 0, v as it is elsewhere"""
    v = np.ascontiguousarray(v, dtype=T)
    with np.errstate(all="ignore"):
        zz = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        s = np.sqrt(zz)
        return np.where((zz > 0)[:, None], v / s[:, None], v).astype(T)


def incidence_angle(nrm, obs, T):
    a, b = normalized(nrm, T), normalized(obs, T)
    with np.errstate(all="ignore"):
        c = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    assert c.dtype == T
    return acos(c.astype(np.float64)).astype(T)


def sphericality(eig, T):
    """(sphericality, unstructureness, structureness) of (n, 3) eigenvalues, in T"""
    e = np.ascontiguousarray(eig, dtype=T)
    with np.errstate(all="ignore"):
        nan_in = np.isnan(e).any(axis=1)
        e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
        e0, e1 = np.where(e0 < e1, e0, e1), np.where(e0 < e1, e1, e0)
        e1, e2 = np.where(e1 < e2, e1, e2), np.where(e1 < e2, e2, e1)
        e0, e1 = np.where(e0 < e1, e0, e1), np.where(e0 < e1, e1, e0)
        tiny = np.finfo(T).tiny
        bad = nan_in | (e2 < tiny) | (e1 < tiny)
        u = e0 / e2
        s = (e1 / e2) * ((e1 - e0) / np.sqrt(e0 * e0 + e1 * e1))
        sph = u - s
    nan = T(np.nan)
    out = [np.where(bad, nan, v).astype(T) for v in (sph, u, s)]
    assert all(v.dtype == T for v in (u, s, sph))
    return out


def cut_keep(v, threshold, use_larger_than, T):
    thr = T(threshold)
    v = np.asarray(v, dtype=T)
    with np.errstate(invalid="ignore"):
        return v <= thr if use_larger_than else v >= thr


def run(xyz, T, stages, knn=KNN, max_dist=np.inf, keep=ALL, desc=None, head_rows=None):
    """pgicp_sensor_chain_ext_*: sensor_chain_ref.run with the three more stages.  (INC,), (SPH, keepU, keepS), (CUT, row, larger,
    threshold) with row a name of CUT_ROWS or an index into desc.  The result carries sensor_chain_ref.run's keys and
    incidence_angles, sphericality, unstructureness, structureness (None: not made)."""
    xyz = np.ascontiguousarray(xyz[:, :3], dtype=T)
    n = len(xyz)
    o = sc.oracle(T)
    h = dict(sc.head(xyz, T, knn, max_dist))
    if head_rows:
        h.update({k: np.ascontiguousarray(v, dtype=T) for k, v in head_rows.items()})
    if desc is not None:
        desc = np.ascontiguousarray(desc, dtype=T)
    rows = dict(normals=h["normals"].copy(), densities=h["densities"], observation_directions=np.zeros((n, 3), T), noise=np.zeros(n, T),
                incidence_angles=np.zeros(n, T), sphericality=np.zeros(n, T), unstructureness=np.zeros(n, T), structureness=np.zeros(n, T))
    made = set()
    cur = np.arange(n, dtype=np.int32)
    arrived, passed, names = [], [], []
    for st in stages:
        name, p = st[0], st[1:]
        names.append(name)
        arrived.append(len(cur))
        if name == OBS:
            rows["observation_directions"][cur] = sc.observation_direction(xyz[cur], p if p else CENTER, T)
            made.add("observation_directions")
        elif name == ORIENT:
            assert OBS in names[:-1] and "normals" in keep
            flip = sc.orient_flips(rows["normals"][cur], rows["observation_directions"][cur], bool(p[0]) if p else True, T)
            rows["normals"][cur[flip]] = -rows["normals"][cur[flip]]
        elif name == SHADOW:
            assert "normals" in keep
            if len(cur):
                cur = cur[o.shadow_keep(xyz[cur], rows["normals"][cur], eps_angle=p[0])]
        elif name == MAXDENS:
            assert "densities" in keep
            if len(cur):
                cur = cur[o.max_density_keep(h["densities"][cur], max_density=p[0], seed=p[1] if len(p) > 1 else 1)]
        elif name == NOISE:
            if len(cur):
                rows["noise"][cur] = o.simple_sensor_noise(xyz[cur], sensor_type=int(p[0]) if p else 0, gain=p[1] if len(p) > 1 else 1.0)
            made.add("noise")
        elif name == INC:
            assert OBS in names[:-1] and "normals" in keep
            rows["incidence_angles"][cur] = incidence_angle(rows["normals"][cur], rows["observation_directions"][cur], T)
            made.add("incidence_angles")
        elif name == SPH:
            assert "eigen_values" in keep
            sph, u, s = sphericality(h["eigen_values"][cur], T)
            rows["sphericality"][cur] = sph
            made.add("sphericality")
            if len(p) > 0 and p[0]:
                rows["unstructureness"][cur] = u
                made.add("unstructureness")
            if len(p) > 1 and p[1]:
                rows["structureness"][cur] = s
                made.add("structureness")
        elif name == CUT:
            if isinstance(p[0], str):
                key = CUT_ROWS[p[0]]
                assert key in made or (key == "densities" and "densities" in keep), p[0]
                v = rows[key][cur]
            else:
                v = desc[cur, int(p[0])]
            cur = cur[cut_keep(v, p[2], bool(p[1]), T)]
        else:
            raise ValueError(name)
        passed.append(len(cur))
    pick = lambda key: rows[key][cur] if key in made else None
    return dict(kept_idx=cur, count=len(cur), xyz=xyz[cur], descriptors=None if desc is None else desc[cur],
                normals=rows["normals"][cur] if "normals" in keep else None, eigen_values=h["eigen_values"][cur] if "eigen_values" in keep else None,
                densities=h["densities"][cur] if "densities" in keep else None, observation_directions=pick("observation_directions"),
                noise=pick("noise"), incidence_angles=pick("incidence_angles"), sphericality=pick("sphericality"),
                unstructureness=pick("unstructureness"), structureness=pick("structureness"), arrived=arrived, passed=passed, names=names)


def median_of(xyz, T, stages, key, keep=ALL, desc=None):
    """the median of the finite values of row `key` (a name of CUT_ROWS) over the points that survive `stages`: a threshold that keeps
    about half of what reaches a cut placed behind them, by construction"""
    v = run(xyz, T, stages, keep=keep, desc=desc)[CUT_ROWS[key]].astype(np.float64)
    v = v[np.isfinite(v)]
    return float(np.median(v)) if len(v) else 1.0


def yaml_list(xyz, T, max_density=None, seed=SEED):
    """the issue's list behind its head -- ObservationDirection, OrientNormals, IncidenceAngle, a cut on incidenceAngles, Sphericality, a
    cut on sphericality, MaxDensity -- with each threshold the median of what reaches its stage"""
    st = [(OBS,) + CENTER, (ORIENT, 1), (INC,)]
    st.append((CUT, "incidence_angles", 1, median_of(xyz, T, st, "incidence_angles")))
    st.append((SPH, 0, 0))
    st.append((CUT, "sphericality", 1, median_of(xyz, T, st, "sphericality")))
    if max_density is None:
        d = run(xyz, T, st)["densities"]
        d = d[np.isfinite(d)]
        max_density = float(np.median(d)) if len(d) else 10.0
    st.append((MAXDENS, max_density, seed))
    return st


def stage_lists(xyz, T, desc=None):
    """name -> stages, thresholds chosen on the reference as medians of what reaches each cut"""
    obs, orient = (OBS,) + CENTER, (ORIENT, 1)
    med = lambda st, key: median_of(xyz, T, st, key, desc=desc)
    full = yaml_list(xyz, T)
    md_of = lambda st: (MAXDENS, med(st, "densities"), SEED)          # a MaxDensity behind `st` at the median density of what reaches it
    sh = (SHADOW, EPS)
    cut_d = (CUT, "densities", 1, med([], "densities"))
    cut_n = (CUT, "simple_sensor_noise", 1, med([(NOISE, 0, 1.0)], "simple_sensor_noise"))
    cs = [obs, orient, sh]
    L = dict(
        inc_alone=[obs, (INC,)], inc_unoriented=[(OBS, 0.5, -0.25, 1.0), (INC,)], sph_alone=[(SPH, 0, 0)], sph_all=[(SPH, 1, 1)],
        sph_uns=[(SPH, 1, 0)], sph_str=[(SPH, 0, 1)],
        cut_alone_dens=[cut_d], cut_alone_dens_smaller=[(CUT, "densities", 0, med([], "densities"))],
        yaml=full,
        cut_ahead_of_shadow_md=[cut_d, obs, orient, sh, md_of([cut_d, obs, orient, sh])],
        cut_behind_shadow_md=cs + [md_of(cs), (SPH, 0, 1), (CUT, "structureness", 1, med(cs + [md_of(cs), (SPH, 0, 1)], "structureness"))],
        md_behind_cut=[(SPH, 0, 0), (CUT, "sphericality", 0, med([(SPH, 0, 0)], "sphericality")),
                       md_of([(SPH, 0, 0), (CUT, "sphericality", 0, med([(SPH, 0, 0)], "sphericality"))])],
        inc_behind_shadow=cs + [(INC,), (CUT, "incidence_angles", 1, med(cs + [(INC,)], "incidence_angles"))],
        two_cuts=[(NOISE, 0, 1.0), (SPH, 1, 1), cut_n, (CUT, "unstructureness", 0, med([(NOISE, 0, 1.0), (SPH, 1, 1), cut_n], "unstructureness"))],
        cut_drops_all=[obs, (INC,), (CUT, "incidence_angles", 1, -1.0), (SPH, 1, 1), md_of([])],
        cut_keeps_all=[obs, (INC,), (CUT, "incidence_angles", 1, 4.0), md_of([])],
        cut_nan_threshold=[(CUT, "densities", 1, float("nan"))],
    )
    return L
