"""CPU: the comparison helpers of tests/gpu_support.py that every GPU test leans on -- what `eq` (by value) and `same_bits`
(dtype, shape, raw bits) accept and refuse, which keys `host_arrays` keeps from the oracle, and the action rows of the rollouts."""
import numpy as np
import pytest

from gpu_support import NOT_STATE, eq, host_arrays, random_actions, same_bits

F32 = np.float32


def _refused(compare, a, b, first):
    """compare(a, b) raises AssertionError; `first`: the index its message must name (None: the refusal comes before any element)"""
    with pytest.raises(AssertionError) as info:
        compare(a, b, "what")
    msg = str(info.value)
    assert msg.startswith("what: ")
    if first is not None:
        assert "first at %s" % np.array(first) in msg, msg
    return msg


def test_eq_names_the_count_the_largest_difference_and_the_first_index():
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    b = a.copy(); b[1, 2] += 0.5
    msg = _refused(eq, a, b, [1, 2])
    assert "1 mismatches" in msg and "max |diff| 5.000e-01" in msg
    eq(a, a.copy(), "equal arrays")


def test_eq_is_a_comparison_by_value():
    nan = np.array([1.0, np.nan, 3.0])
    _refused(eq, nan, nan.copy(), [1])                          # NaN is unequal to NaN
    eq(np.array([0.0, -0.0], F32), np.array([-0.0, 0.0], F32), "signed zeros are equal by value")


def test_same_bits_sees_what_a_value_comparison_does_not():
    _refused(same_bits, np.array([1.0, -0.0, 2.0], F32), np.array([1.0, 0.0, 2.0], F32), [1])
    one = np.ones((2, 3), F32)
    ulp = one.copy(); ulp[1, 1] = np.nextafter(F32(1.0), F32(2.0))
    _refused(same_bits, one, ulp, [1, 1])
    nan = np.array([np.nan, np.inf, -0.0])
    same_bits(nan, nan.copy(), "a NaN has the bits it has")


def test_same_bits_wants_equal_dtype_and_shape_first():
    msg = _refused(same_bits, np.array([1, 2], np.int32), np.array([1, 2], np.int64), None)
    assert "int32" in msg and "int64" in msg
    _refused(same_bits, np.array([1.0, 2.0], F32), np.array([1.0, 2.0], np.float64), None)
    _refused(same_bits, np.zeros((2, 3), F32), np.zeros((3, 2), F32), None)
    _refused(same_bits, np.zeros(3, F32), np.zeros((3, 1), F32), None)
    eq(np.array([1, 2], np.int32), np.array([1.0, 2.0]), "eq does not look at the dtype")


class _Tensor:
    """What host_arrays asks of a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_host_arrays_drops_the_four_device_only_keys():
    assert NOT_STATE == ("field", "field_overflow", "rect_table", "rect_index")
    keys = NOT_STATE + ("robot_pose", "costmap", "counters", "ped_waypoints", "scan_threshold")
    occ = np.zeros((1, 8, 8), np.uint8); occ[0, 3, 4] = 1
    host = host_arrays({k: _Tensor(np.full(2, i)) for i, k in enumerate(keys)}, occ)
    assert set(host) == set(keys) - {"field_overflow", "rect_table", "rect_index"}
    for i, k in enumerate(keys):
        if k not in NOT_STATE:
            assert np.array_equal(host[k], np.full(2, i)), k
    assert host["field"].dtype == F32 and host["field"].shape == occ.shape        # the oracle's own field of occ
    assert host["field"][0, 3, 4] == 0.0 and host["field"][0, 3, 0] == 4.0


# test_gpu_autoreset.py's _actions(rng, cfg, t) before the rows moved here: default_rng(1), three arenas, t = 0 .. 7.  The rollouts are
# tuned to reach crashes and resets with exactly these draws; the burst at t = 3 still consumes its draws.
ACTIONS = [
    [[0.25591081235012836, 0.5742712923356722], [0.47523184816296765, -0.24085574142657862], [0.07207980635981687, -0.09814214531510312]],
    [[0.4138512969102209, -0.6047243350488725], [0.20459956818458064, 0.3244967791037524], [0.27479684383652975, 0.04882344092067614]],
    [[0.16486585824954608, -0.059522701464766126], [0.39421435171420216, -0.4684266275236291], [0.1515974146458225, -0.12401537734767454]],
    [[0.5, 0.0], [0.5, 0.0], [0.5, 0.0]],
    [[0.4808285968318934, -0.28557925882192536], [0.3623949703867668, -0.4343654287678376], [0.2706134277737171, 0.6015045289166497]],
    [[0.25803429277393936, 0.35415438635814145], [0.05793280623538516, 0.14464422534789179], [0.3117448777687502, 0.5341410621323553]],
    [[0.01979643833210143, -0.5601925386881592], [0.2642946316300108, 0.1809000564983999], [0.22966794144270186, 0.4513700332552407]],
    [[0.296470509052142, 0.012154728347531951], [0.1300487238686116, 0.013937772117162295], [0.4199407605157044, 0.32387866585878766]],
]


def test_random_actions_are_the_rows_the_rollouts_were_tuned_on():
    rng = np.random.default_rng(1)
    for t, want in enumerate(ACTIONS):
        same_bits(random_actions(rng, 3, t), np.array(want), "step %d" % t)
    rng, bursts = np.random.default_rng(1), np.random.default_rng(1)
    for t in range(8):                                          # t = None: the same draws without the bursts
        plain, burst = random_actions(rng, 3), random_actions(bursts, 3, t)
        assert (plain[:, 0] < 0.5).all()
        if t != 3:
            same_bits(plain, burst, "step %d without bursts" % t)
