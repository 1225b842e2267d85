"""A plain reference of the three transformation checkers of the ICP loop -- Counter, Differential, Bound -- written from their
definition (SURVEY.md A.9 and libpointmatcher's description of them), in numpy float64.  TEST INFRASTRUCTURE ONLY.

It shares nothing with the product's checker_check (icp_math.hpp) or the oracle's orc_checker_check (icp_oracle.c):
  * the history is an unbounded Python list of 4x4 matrices -- no ring, no capacity, no shift;
  * a rotation distance is the angle of R_i R_{i-1}^T read off the rotation MATRIX through atan2 (half the norm of its skew part
    against half of trace - 1), not the quaternion product the other two use.

The definition:
  Counter{maxIterationCount}     counts the checks; at the limit it stops the loop and raises the max-iterations condition.
  Differential{minDiffRotErr, minDiffTransErr, smoothLength}
                                 keeps every T_iter it was shown, the initial identity included.  Once it holds more than
                                 smoothLength of them: the mean, over the last smoothLength steps, of the rotation distance and
                                 of the norm of the translation difference between consecutive entries.  Both means strictly
                                 below their limits: stop ("converged").  A mean that is NaN: ConvergenceError.
  Bound{maxRotationNorm, maxTranslationNorm}
                                 rotation distance / translation norm of T_iter from what the checkers were initialised with
                                 (the identity).  Strictly above a limit: ConvergenceError.  A limit <= 0: not looked at.
They run in that order.  The Counter's stop leaves the check before the Bound is looked at, so it is never turned into an
error; Counter and Differential may both stop the loop on the same iteration (both flags are then set)."""
import math

import numpy as np

OK, ERR_NAN, ERR_BOUND = 0, 2, 7           # the status numbers of include/pgicp.h (and of the oracle)


def rotation_angle(Ra, Rb):
    """angle in [0, pi] of the rotation Ra Rb^T, from the matrix"""
    D = np.asarray(Ra, dtype=np.float64) @ np.asarray(Rb, dtype=np.float64).T
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    c = 0.5 * (D[0, 0] + D[1, 1] + D[2, 2] - 1.0)
    if math.isnan(s) or math.isnan(c):
        return math.nan
    return math.atan2(s, c)


def step_sizes(T_iters):
    """(rotation distance, translation distance) between consecutive entries of [I, T_1, T_2, ...]: entry k - 1 is the step
    that iteration k made"""
    hist = [np.eye(4)] + [np.asarray(T, dtype=np.float64).reshape(4, 4) for T in T_iters]
    rot = [rotation_angle(hist[i][:3, :3], hist[i - 1][:3, :3]) for i in range(1, len(hist))]
    trans = [float(np.linalg.norm(hist[i][:3, 3] - hist[i - 1][:3, 3])) for i in range(1, len(hist))]
    return np.array(rot), np.array(trans)


def smoothed_series(T_iters, smooth):
    """{iteration k (1-based): (mean rotation step, mean translation step) over iterations k - smooth + 1 .. k} for every k
    at which the Differential checker has a mean to look at, i.e. k >= smooth"""
    rot, trans = step_sizes(T_iters)
    return {k: (float(np.mean(np.abs(rot[k - smooth:k]))), float(np.mean(np.abs(trans[k - smooth:k]))))
            for k in range(smooth, len(rot) + 1)}


def bound_series(T_iters):
    """{iteration k: (rotation distance of T_k from the identity, norm of its translation)}: what the Bound checker compares"""
    out = {}
    for k, T in enumerate(T_iters, start=1):
        T = np.asarray(T, dtype=np.float64).reshape(4, 4)
        out[k] = (rotation_angle(T[:3, :3], np.eye(3)), float(np.linalg.norm(T[:3, 3])))
    return out


def check(history, count, max_iters, min_rot, min_trans, smooth, bound_rot=0.0, bound_trans=0.0):
    """one look of the three checkers at history[-1] (history = [I, T_1, ..., T_count]).  Returns the set of what happened:
    "counter", "differential" (stops), "nan", "bound" (errors); empty: go on."""
    out = set()
    if count >= max_iters:
        out.add("counter")
    if len(history) > smooth:
        rot = [abs(rotation_angle(history[i][:3, :3], history[i - 1][:3, :3])) for i in range(len(history) - smooth, len(history))]
        trans = [float(np.linalg.norm(history[i][:3, 3] - history[i - 1][:3, 3])) for i in range(len(history) - smooth, len(history))]
        mr, mt = sum(rot) / smooth, sum(trans) / smooth
        if math.isnan(mr) or math.isnan(mt):
            return {"nan"}
        if mr < min_rot and mt < min_trans:
            out.add("differential")
    if "counter" not in out and (bound_rot > 0.0 or bound_trans > 0.0):
        T = history[-1]
        r, t = rotation_angle(T[:3, :3], np.eye(3)), float(np.linalg.norm(T[:3, 3]))
        if (bound_rot > 0.0 and r > bound_rot) or (bound_trans > 0.0 and t > bound_trans):
            return {"bound"}
    return out


def run(T_iters, max_iters, min_rot, min_trans, smooth, bound_rot=0.0, bound_trans=0.0):
    """The ICP loop's control over a recorded trajectory T_iters[k - 1] = T_iter after iteration k.
    Returns (iterations, converged, max_iter_reached, status).  The trajectory must reach the stop."""
    history = [np.eye(4)]
    for k, T in enumerate(T_iters, start=1):
        history.append(np.asarray(T, dtype=np.float64).reshape(4, 4))
        f = check(history, k, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans)
        if "nan" in f:
            return k, False, False, ERR_NAN
        if "bound" in f:
            return k, False, False, ERR_BOUND
        if f:
            return k, "differential" in f, "counter" in f, OK
    raise ValueError("checkers_ref.run: the trajectory ends before the checkers stop the loop")


def margin(T_iters, iterations, min_rot, min_trans, smooth, bound_rot=0.0, bound_trans=0.0):
    """the smallest relative distance, over iterations 1 .. `iterations`, between a value the checkers compare and the limit
    they compare it with (limits <= 0 are not compared: min_diff = 0 can never be undercut, a bound of 0 is off)"""
    sm, bd = smoothed_series(T_iters, smooth), bound_series(T_iters)
    worst = math.inf
    for k in range(1, iterations + 1):
        pairs = []
        if k in sm:
            pairs += [(sm[k][0], min_rot), (sm[k][1], min_trans)]
        pairs += [(bd[k][0], bound_rot), (bd[k][1], bound_trans)]
        for value, limit in pairs:
            if limit > 0.0:
                worst = min(worst, abs(value - limit) / limit)
    return worst


def between(a, b):
    """the margin rule: a limit is the geometric mean of two adjacent values of the series it is compared with"""
    assert a > 0.0 and b > 0.0 and a != b
    return math.sqrt(a * b)
