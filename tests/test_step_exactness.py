"""What the shorter finish of a scanned ray rests on (kernels_step.hpp ray_result, navsim_device.hpp gauss_noise).

The fused step computes a hit range from integers and the scan noise without the compiler's denormal handling of logf.
Both are exact rewrites, not approximations: these tests pin the arguments over their whole domains, so that a compiler or
a map-size change that breaks one fails here instead of as a changed observation somewhere in a long run."""
import numpy as np
import pytest

KMAX = 1448        # kernels_step.hpp kIntRangeMaxSide


def test_integer_hit_range_domain():
    """CPU: on a map of at most KMAX cells a side, a hit cell's offset (ix, iy) from the scan origin (both cells of the map)
    has ix^2 + iy^2 < 2^22, where float32 holds the squares and their sum exactly and nv::sqrt_small_int is IEEE sqrtf
    (tests/test_gpu_parity.py checks that on all of [0, 2^22))."""
    def bound(n):
        return 2 * (n - 1) ** 2
    assert bound(KMAX) < 1 << 22
    # float32 evaluation of the replaced form equals the integer on the extreme offsets
    o = np.arange(-(KMAX - 1), KMAX, dtype=np.int64)
    f = o.astype(np.float32)
    s = f * f + np.float32((KMAX - 1) ** 2)
    assert np.array_equal(s.astype(np.int64), o * o + (KMAX - 1) ** 2)


@pytest.mark.gpu
def test_integer_hit_range_is_sqrtf_on_every_offset():
    """GPU: debug function 15 evaluates the step's integer hit range and the float32 sqrtf form it replaced for every
    offset (ix, iy) in [-1447, 1447]^2 -- all a map of at most KMAX cells a side can produce; 0 = bit-identical."""
    import torch
    from nav_gym_amd import lib, sim
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    lib.load()
    n = 2895 * 2895
    x = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    bad = sim.debug_math(15, x)
    assert int(bad.sum()) == 0, "%d offsets differ" % int(bad.sum())


@pytest.mark.gpu
def test_noise_pieces_bit_identical_on_every_input():
    """GPU: debug function 16 compares, for every 24-bit value m a hash can give, nv::log_normal(u1) with the compiler's
    __logf(u1), u1 = (m + 1) 2^-24, and the folded angle m * (6.28318530718f 2^-24) with 6.28318530718f * (m 2^-24):
    the noise formula's only two rewritten pieces, each on its full input set."""
    import torch
    from nav_gym_amd import lib, sim
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    lib.load()
    x = torch.zeros(1 << 24, dtype=torch.float64, device="cuda:0")
    bad = sim.debug_math(16, x)
    assert int(bad.sum()) == 0, "%d inputs differ" % int(bad.sum())
