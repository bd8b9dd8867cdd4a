"""CPU: scan ground truth (include/navsim.h navsim_scan_labels) -- the entry's place in the C ABI, its argument refusals, the
keyword on NavGymEnv, the specification (tests/scan_labels_spec.py) against the oracle's own scan on moving worlds, and hand-made
scenes with known answers.  The device against that specification is tests/test_gpu_scan_labels.py."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import ref
import scan_labels_spec as spec
from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structure_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()         # no structure changed its size
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert re.search(r"\bint navsim_scan_labels\(", header)
    assert "navsim_scan_labels" in abi.EXPORTS and hasattr(L, "navsim_scan_labels")
    fields = struct_fields(header, "navsim_scan_labels_out")
    assert fields == ["range", "label", "index", "hits"]
    assert [n for n, _ in abi.NavsimScanLabelsOut._fields_] == fields == list(abi.SCAN_LABELS_OUT)
    assert C.sizeof(abi.NavsimScanLabelsOut) == 4 * C.sizeof(C.c_void_p)
    for name, value in (("NONE", 0), ("WALL", 1), ("PED_BODY", 2), ("PED_LEG", 3)):
        assert getattr(abi, "BEAM_" + name) == value and re.search(r"#define NAVSIM_BEAM_%s\s+%d\b" % (name, value), header)
    assert "oracle/navsim_ref.c:557-631" in header                               # the arithmetic the rule cites


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, max_peds=4, ped_model=abi.PED_SFM, map_h=16, map_w=16, n_beams=8)
    st_fields = ("robot_pose", "field", "n_peds", "ped_pose", "ped_dist", "ped_has_legs")

    def state(skip=(), **more):
        st = abi.NavsimState()
        for k in st_fields:
            setattr(st, k, None if k in skip else ptr)
        for k, v in more.items():
            setattr(st, k, v)
        return st

    def outputs(skip=()):
        o = abi.NavsimScanLabelsOut()
        for k in abi.SCAN_LABELS_OUT:
            setattr(o, k, None if k in skip else ptr)
        return o

    ref_ = lambda x: None if x is None else C.byref(x)
    call = lambda c=cfg, s=state(), o=outputs(): L.navsim_scan_labels(ref_(c), ref_(s), None, ref_(o), None)

    def changed(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert call(c=None) == call(s=None) == call(o=None) == abi.E_ARG
    for k in ("range", "label", "index"):
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    for k in st_fields:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
    for k, bad in (("n_envs", -1), ("n_beams", 0), ("max_peds", 0), ("max_peds", 65), ("max_peds", -1), ("map_h", 0), ("map_w", 0),
                   ("march_rule", 3), ("march_rule", -1)):
        assert call(c=changed(**{k: bad})) == abi.E_ARG, (k, bad)
    assert call(c=changed(ped_model=abi.PED_NONE, max_peds=-1)) == abi.E_ARG
    assert call(c=changed(shared_field=1), s=state(map_slot=ptr)) == abi.E_ARG
    assert call(c=changed(field_format=2)) == abi.E_UNSUPPORTED
    assert call(c=changed(field_format=abi.FIELD_F32), s=state(rect_table=ptr)) == abi.E_UNSUPPORTED     # records need the packed field
    assert call(c=changed(field_format=abi.FIELD_U16T, map_h=1032), s=state(rect_table=ptr)) == abi.E_UNSUPPORTED
    assert call(c=changed(angle_min=-3.2, angle_last=3.2)) == abi.E_UNSUPPORTED   # wider than 2 pi with pedestrians to merge
    assert call(c=changed(n_beams=10240)) == abi.E_UNSUPPORTED                    # 16 B per beam: beyond a compute unit's 160 KB of LDS
    assert call(c=changed(n_beams=10000, n_envs=0)) == abi.OK
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted
    assert call(c=changed(n_envs=0, max_peds=64)) == abi.OK
    assert call(c=changed(n_envs=0), o=outputs(skip=("hits",))) == abi.OK         # (hits may be NULL)
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, max_peds=0), s=state(skip=st_fields[2:])) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, angle_min=-3.2, angle_last=3.2)) == abi.OK


# ---- the keyword on NavGymEnv -------------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, scan_labels=True)
    assert env.scan_labels_on is True and [p.key for p in env._products] == ["scan_labels"]
    assert env._products[0].keys == ("range", "label", "index", "hits")
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.scan_labels_on is True and twin.num_envs == 3
    with pytest.raises(RuntimeError):
        env.scan_labels()                                  # before reset()
    for model in ("orca", "external"):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, scan_labels=True, pedestrian_model=model).scan_labels_on
    none = nav_gym_env.make("NavGym-v0", num_envs=3, scan_labels=True, pedestrian_model="none")
    assert none._products[0].keys == ("range", "label", "index")                  # hits: only with a pedestrian model
    both = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, scan_labels=True, observe_local_map=8)
    assert [p.key for p in both._products] == ["local_map", "scan_labels"]       # one more row, after the local map
    for bad in (1, 0, "yes", None, 2.0):
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, scan_labels=bad)
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.scan_labels_on is False and plain._products == []
    with pytest.raises(RuntimeError):
        plain.scan_labels()
    assert "scan_labels" not in registry.spec("NavGym-v0")["kwargs"]


def test_output_layout():
    from nav_gym_amd import sim
    lay = sim.blob_layout(abi.SCAN_LABELS_OUT, 5, {"B": 7, "N": 3})
    assert [(k, d, shape) for k, d, _, _, shape in lay[:-1]] == [
        ("range", "float32", (5, 7)), ("label", "uint8", (5, 7)), ("index", "int8", (5, 7)), ("hits", "int32", (5, 3))]
    assert [hi - lo for _, _, lo, hi, _ in lay[:-1]] == [140, 35, 35, 60]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))
    assert [k for k, *_ in sim.blob_layout(abi.SCAN_LABELS_OUT, 5, {"B": 7, "N": 3}, omit=("hits",))[:-1]] == ["range", "label", "index"]


# ---- the specification against the oracle's own scan ---------------------------------------------------------------------------
@pytest.mark.parametrize("E,size,N,lidar,seed", spec.ORACLE_WORLDS, ids=lambda v: str(v))
def test_spec_range_is_the_oracle_scan(E, size, N, lidar, seed):
    """Arenas of hand-built worlds, pedestrians 0.5 - 5 m from the robot, half of them with legs, driven by random commands
    (NAVSIM_PED_EXTERNAL), noise off: after navsim_reset_obs and after each of three steps the specification's `range` is the
    newest scan slot of the oracle's observation, bit for bit.  The 600-cell world (30 m) is wider than range_max = 25 m and has
    no wall around it: it has beams without a return.  Conditions on the test's own inputs: every class a world is meant to show
    is there (the populations are printed)."""
    cfg = spec.config(E, N, size, lidar=lidar, n_scan_stack=2)
    far = size * cfg.resolution > cfg.range_max
    occ, scenes = spec.random_scenes(E, N, size, seed, wall=not far)
    fields = ref.build_dt(occ)
    r = ref.RefSim(cfg, dict(spec.scene_world(cfg, scenes), field=fields))
    rng = np.random.default_rng(seed)
    count = np.zeros(4, int)
    none_per_snapshot = []
    obs = r.reset_obs()
    for t in range(4):
        if t:
            r.set_ped_cmd(np.stack([rng.uniform(0.0, 0.6, (E, N)), rng.uniform(-0.6, 0.6, (E, N))], axis=2))
            obs, _ = r.step(np.stack([rng.uniform(0.0, 0.3, E), rng.uniform(-0.5, 0.5, E)], axis=1))
        o = spec.answer(r.cfg, fields, r.a)
        assert o["range"].dtype == np.float32
        assert np.array_equal(o["range"].view(np.uint32), spec.newest_scan(cfg, obs).view(np.uint32)), "snapshot %d" % t
        assert o["hits"].sum() == (o["index"] >= 0).sum()
        assert ((o["index"] >= 0) == (o["label"] >= spec.BODY)).all() and (o["index"] < N).all()
        assert ((o["label"] == spec.NONE) == (o["range"] == np.float32(cfg.range_max))).all()
        count += np.bincount(o["label"].reshape(-1), minlength=4)
        none_per_snapshot.append(int((o["label"] == spec.NONE).sum()))
    print("beams by label over four snapshots:", count.tolist(), "without a return per snapshot:", none_per_snapshot)
    assert count[spec.WALL] > 0 and count[spec.BODY] > 0 and count[spec.LEG] > 0
    if far:
        assert min(none_per_snapshot) > 400
    else:
        assert count[spec.NONE] == 0


# ---- hand-made scenes with known answers: an empty walled room, the robot at its centre looking along +x ------------------------
CENTRE = 32                                                # of 64 beams over the full circle: the one that looks straight ahead


def test_scene_body_straight_ahead():
    cfg, _, _, o = spec.hand_scene([spec.ahead(2.0)], lidar=64)
    assert (o["label"][0, CENTRE], o["index"][0, CENTRE]) == (spec.BODY, 0)
    assert abs(float(o["range"][0, CENTRE]) - 1.78) < 1e-3                       # the near side of the 0.44 m deep rectangle
    assert o["hits"].tolist() == [[int((o["index"] == 0).sum())]] and o["hits"][0, 0] >= 1
    assert (o["label"][o["index"] < 0] == spec.WALL).all()                      # every other beam ends on the room's wall


def test_scene_legs_take_a_few_beams():
    cfg, _, _, o = spec.hand_scene([spec.ahead(2.0, legs=1)], lidar=None)        # 1081 beams: 0.25 degrees apart
    leg = o["label"][0] == spec.LEG
    assert 1 <= leg.sum() <= 24 and (o["index"][0, leg] == 0).all() and not (o["label"] == spec.BODY).any()
    k = np.flatnonzero(leg)
    assert o["label"][0, k.min() - 1] == spec.WALL and o["label"][0, k.max() + 1] == spec.WALL    # the neighbours see the wall
    assert o["hits"].tolist() == [[int(leg.sum())]]
    cfg, _, _, o = spec.hand_scene([spec.ahead(2.0, legs=1)], lidar=None, lidar_legs=0)            # legs not rendered: the body
    assert (o["label"][0, 540], o["index"][0, 540]) == (spec.BODY, 0) and not (o["label"] == spec.LEG).any()


def test_scene_two_on_one_bearing_the_nearer_wins():
    for peds, near in (([spec.ahead(3.0), spec.ahead(1.5)], 1), ([spec.ahead(1.5), spec.ahead(3.0)], 0)):
        cfg, _, _, o = spec.hand_scene(peds, lidar=64)
        assert o["index"][0, CENTRE] == near and abs(float(o["range"][0, CENTRE]) - 1.28) < 1e-3


def test_scene_behind_a_wall_and_behind_the_lidar():
    # a pedestrian whose centre lies 0.5 m inside... beyond the room's wall: the wall's face is nearer on every beam
    cfg, _, _, o = spec.hand_scene([((spec.ROBOT[0] + 4.9625 + 0.5, spec.ROBOT[1], 0.0), 0)], lidar=64)
    assert o["hits"].tolist() == [[0]] and (o["index"] == -1).all() and (o["label"] == spec.WALL).all()
    # 2 m behind a 270-degree lidar that looks along +x: no beam points there
    cfg, _, _, o = spec.hand_scene([spec.ahead(-2.0)], lidar=None)
    assert o["hits"].tolist() == [[0]] and (o["label"] == spec.WALL).all()


def test_scene_across_the_seam_of_a_full_circle():
    cfg, _, _, o = spec.hand_scene([spec.ahead(-1.5)], lidar=64)                  # bearing pi: beams 0 and 63 are its neighbours
    assert o["label"][0, 0] == spec.BODY and o["label"][0, 63] == spec.BODY and o["index"][0, 0] == o["index"][0, 63] == 0
    assert o["label"][0, CENTRE] == spec.WALL


def test_scene_rectangle_around_the_lidar():
    cfg, _, _, o = spec.hand_scene([spec.ahead(0.05, side=0.03, yaw=0.4)], lidar=64)
    assert (o["label"] == spec.BODY).all() and (o["index"] == 0).all() and o["hits"].tolist() == [[64]]
    assert float(o["range"].max()) < 0.5


def test_scene_range_max_below_a_pedestrian():
    cfg, _, _, o = spec.hand_scene([spec.ahead(4.0)], lidar=64, range_max=3.0)
    assert (o["label"] == spec.NONE).all() and (o["index"] == -1).all() and (o["range"] == np.float32(3.0)).all()
    assert o["hits"].tolist() == [[0]]
    cfg, _, _, o = spec.hand_scene([spec.ahead(2.0)], lidar=64, range_max=3.0)    # ... and one inside it
    assert (o["label"][0, CENTRE], o["index"][0, CENTRE]) == (spec.BODY, 0) and (o["label"] != spec.WALL).all()


def test_scene_skip_and_single_beam():
    cfg, _, _, o = spec.hand_scene([spec.ahead(2.0)], lidar=64, skip=[1])
    assert not o["range"].any() and not o["label"].any() and (o["index"] == -1).all() and not o["hits"].any()
    cfg, _, _, o = spec.hand_scene([spec.ahead(-2.0)], lidar=1)                   # B == 1: the one beam looks along -pi
    assert o["range"].shape == (1, 1) and (o["label"][0, 0], o["index"][0, 0]) == (spec.BODY, 0) and o["hits"].tolist() == [[1]]
    cfg, _, _, o = spec.hand_scene([], lidar=64, ped_model=abi.PED_NONE)          # no pedestrian model: walls alone
    assert (o["label"] == spec.WALL).all() and (o["index"] == -1).all()
