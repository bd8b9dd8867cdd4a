"""CPU: sim.blob_layout, the one carve behind ped_observation_layout / goal_path_layout / dwa_layout and the local map's buffer,
on a made-up table: a symbolic extent, an omitted name, a zero-size array."""
import numpy as np

from nav_gym_amd import abi, sim


def test_blob_layout_on_a_made_up_table():
    table = {"wide": ("float64", ("K", 3)), "flag": ("uint8", ()), "gone": ("int32", ("K",)), "empty": ("float32", (0, 2)),
             "tail": ("int32", ("N",)), "last": ("uint8", (3,))}
    E, K, N = 5, 3, 7
    lay = sim.blob_layout(table, E, {"K": K, "N": N}, omit=("gone",))
    assert [row[0] for row in lay] == ["wide", "flag", "empty", "tail", "last", None]
    want = dict(wide=("float64", (E, K, 3)), flag=("uint8", (E,)), empty=("float32", (E, 0, 2)), tail=("int32", (E, N)), last=("uint8", (E, 3)))
    end_before = 0
    for name, dtype, lo, hi, shape in lay[:-1]:
        assert (dtype, shape) == want[name]
        assert lo % 16 == 0 and lo >= end_before, name                         # aligned, and behind the array before it
        assert hi - lo == int(np.prod(shape)) * np.dtype(dtype).itemsize, name
        end_before = hi
    assert lay[2][2] == lay[2][3]                                              # the zero-size array takes no byte
    total = (end_before + 15) // 16 * 16
    assert lay[-1] == (None, None, total, max(total, 16), None) and total == 368 + 16 + 0 + 144 + 16
    # nothing but zero-size arrays: still an allocation of 16 bytes
    assert sim.blob_layout(table, 0, {"K": K, "N": N})[-1] == (None, None, 0, 16, None)
    assert sim.blob_layout({}, E)[-1] == (None, None, 0, 16, None)
    # the three public layouts are this function on abi's tables
    assert sim.ped_observation_layout(E, K, N) == sim.blob_layout(abi.PED_OBSERVATION, E, {"K": K, "N": N})
    assert sim.goal_path_layout(E) == sim.blob_layout(abi.GOAL_PATH_OUT, E)
    assert sim.dwa_layout(E, 6, scores=True) == sim.blob_layout(abi.DWA_OUT, E, {"C": 6})
    assert sim.dwa_layout(E, 6) == sim.blob_layout(abi.DWA_OUT, E, {"C": 6}, omit=("scores", "first_hit"))
