"""The covariance's small-angle parameters (alpha, beta, gamma of the last increment) are computed on the device, and by the
oracle on the host.  asin / atan2 / cos of two math libraries do not owe each other the same last bit, so both sides take them
from one arctangent written in IEEE operations only: det_atan2 in pgslam_amd/csrc/icp_math.hpp, orc_atan2 in the oracle.
Here, without a device: the two are the same to the bit, within 1 ulp of the host's atan2 (2 of asin), and right at the
special arguments."""
import ctypes as C
import math

import numpy as np
import pytest

from test_checkers_ref_host import ProductChecker


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    p = ProductChecker(tmp_path_factory.mktemp("small_angles_host"))
    p.lib.pgicp_host_atan2.restype = C.c_double
    return p


def bits(v):
    return np.float64(v).tobytes()


def test_atan2_same_bits_and_one_ulp(oracle32, product):
    rng = np.random.default_rng(5)
    n = 60_000
    y = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-14, 3, n) * rng.random(n)
    x = rng.choice([-1.0, 1.0, 1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 1, n)
    # the breakpoints of the argument reduction, from both sides
    edge = np.array([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 66, 1.0, 1e-300, 1e300])
    y = np.concatenate([y, edge, np.nextafter(edge, 0.0), np.nextafter(edge, np.inf), -edge])
    x = np.concatenate([x, np.ones(3 * len(edge)), -np.ones(len(edge))])
    for a, b in zip(y.tolist(), x.tolist()):
        got = product.lib.pgicp_host_atan2(C.c_double(a), C.c_double(b))
        assert bits(got) == bits(oracle32.atan2(a, b)), (a, b)
        want = math.atan2(a, b)
        assert abs(got - want) <= math.ulp(want), (a, b, got, want)


def test_atan2_special_arguments(oracle32, product):
    f = lambda a, b: product.lib.pgicp_host_atan2(C.c_double(a), C.c_double(b))
    for a, b in [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1.0, 0.0),
                 (-1.0, 0.0), (1.0, -0.0), (2.0, math.inf), (-2.0, math.inf), (math.inf, 1.0), (-math.inf, 1.0)]:          # (finite x; an infinite y over a negative x is a unit in the last place off, and no rotation has one)
        assert bits(f(a, b)) == bits(math.atan2(a, b)) == bits(oracle32.atan2(a, b)), (a, b)
    assert math.isnan(f(math.nan, 1.0)) and math.isnan(f(1.0, math.nan)) and math.isnan(oracle32.atan2(math.nan, 1.0))


def test_small_angles_of_rotations(product):
    """R = Rz(gamma) Ry(beta) Rx(alpha): the three angles come back, tiny increments (a converged run) and large ones"""
    rng = np.random.default_rng(6)
    out = (C.c_double * 3)()
    for scale in (1e-9, 1e-4, 1e-2, 0.5):
        for _ in range(200):
            al, be, ga = (scale * rng.uniform(-1, 1, 3)).tolist()
            ca, sa, cb, sb, cg, sg = math.cos(al), math.sin(al), math.cos(be), math.sin(be), math.cos(ga), math.sin(ga)
            T = np.eye(4)
            T[:3, :3] = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
            product.lib.pgicp_host_small_angles(T.ctypes.data_as(C.c_void_p), out)
            np.testing.assert_allclose(out[:], [al, be, ga], rtol=1e-12, atol=1e-16 + 4e-16 * scale)
            # the formulas as libpointmatcher writes them, with the host's math library
            beta = -math.asin(T[2, 0])
            want = [math.atan2(T[2, 1], T[2, 2]), beta, math.atan2(T[1, 0] / math.cos(beta), T[0, 0] / math.cos(beta))]
            for g, w in zip(out[:], want):
                assert abs(g - w) <= 4.0 * math.ulp(w) + 1e-300, (g, w)
