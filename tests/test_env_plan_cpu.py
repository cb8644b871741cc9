"""CPU: plan_env (uhc_amd/csrc/uhc_env_plan.h), the part of uhc_env_create that decides what an env is -- the humanoid's extents in front of the objects, hinge
or ball, the observation's width, every refusal -- compiled with the host compiler (tests/env_plan_probe.cpp) and run on the dims the project uses.  The widths
are compared with two sources that do not read the header: the literals the GPU tests assert on the device, and the length of the vector the oracle
(oracle/env_oracle.py) returns for the same version and flags."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import probe_build
from uhc_amd._capi import UhcEnvDesc, env_desc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INTS = ("n_obj", "nqh", "nvh", "nbh", "ball", "has_shape", "obs_v", "reward_v", "obs_flags", "term_body", "obs_dim", "fut_frames", "fut_skip", "env_episode_len",
        "expert_trail_steps", "ee0", "ee1", "ee2", "ee3", "ee4", "n_env", "nq", "nv", "nu", "nbody", "action_dim", "vf_dim")
HINGE = dict(n_env=2, nq=76, nv=75, nu=69, nbody=25, action_dim=105, vf_dim=6, n_trailing_free=0)  # the asset humanoid
BALL = dict(HINGE, nq=99)                                                                           # its ball-joint variant
DIMS_TEXT = ("uhc_env_create: hinge humanoid (free root + scalar joints) or ball-joint humanoid (free root + one ball joint per body), followed by num_obj free bodies, "
             "nq <= 192, expected")
NUM_OBJ_TEXT = "uhc_env_create: num_obj exceeds the free bodies at the end of the model"
BALL_TEXT = "uhc_env_create: the ball-joint env has observation v2 (get_full_obs_v2_quat) and reward 0 (world_rfc_implicit_quat)"
FUT_TEXT = "uhc_env_create: obs_v 3 needs 1 <= fut_frames <= 64, skip >= 0"
OBS_V_TEXT = "uhc_env_create: obs_v must be 0 .. 6"
REWARD_V_TEXT = "uhc_env_create: reward_v must be 0 .. 5 (implicit, explicit, implicit_v1_mul, explicit_mul, implicit_v2, implicit_v3)"
TERM_TEXT = "uhc_env_create: term_body must be 0 (cfg.env_term_body 'body') or 1 ('root')"


def with_objects(dims, k=2):
    """the same humanoid with k free bodies behind it (7 qpos, 6 qvel, one body each)"""
    return dict(dims, nq=dims["nq"] + 7 * k, nv=dims["nv"] + 6 * k, nbody=dims["nbody"] + k, n_trailing_free=k)


@pytest.fixture(scope="module")
def probe():
    L = C.CDLL(probe_build.build_probe("env_plan_probe.so", ["tests/env_plan_probe.cpp"],
                                       ["uhc_amd/csrc/uhc_env_plan.h", "uhc_amd/csrc/uhc_device_env.h", "include/uhc_amd.h"]))
    L.uhc_env_plan_probe.argtypes = [C.POINTER(C.c_int), C.c_double, C.POINTER(C.c_double), C.POINTER(UhcEnvDesc), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int), C.c_char_p, C.c_int]

    def plan(dims, desc):
        """-> (the plan's ints by name + "doubles", None), or (None, the refusal's text)"""
        d = (C.c_int * 8)(*[dims[k] for k in ("n_env", "nq", "nv", "nu", "nbody", "action_dim", "vf_dim", "n_trailing_free")])
        ints, dbl, ptrs, err = (C.c_int * len(INTS))(), (C.c_double * 22)(), C.c_int(-1), C.create_string_buffer(512)
        if L.uhc_env_plan_probe(d, 1.0 / 30, (C.c_double * 4)(0.7071, -0.7071, 0.0, 0.0), C.byref(desc), ints, dbl, C.byref(ptrs), err, 512):
            return None, err.value.decode()
        assert ptrs.value == 0  # (the plan is the scalar part: every pointer is still null)
        return dict(zip(INTS, ints), doubles=list(dbl)), None

    return plan


@pytest.fixture(scope="module")
def oracle_len():
    """the length of the oracle's observation for (ball, obs_v, flags ...), from the state and the expert window of the golden clips' first frames: the calls of
    tests/test_gpu_env.py::_oracle_obs and of tests/test_gpu_env_objects.py's obs_of, on the CPU"""
    import torch
    from oracle import env_oracle as E
    from uhc_amd.sim import load_asset_model
    from uhc_amd.smpllib.torch_smpl_humanoid import Humanoid
    f = np.load(os.path.join(G, "g3_qpos_fk.npz"))
    g = np.load(os.path.join(G, "g14_ball_env.npz"))
    model = load_asset_model()
    hinge = Humanoid(model=model).qpos_fk(torch.from_numpy(f["f_qpos"][:12].copy()))
    ball = Humanoid(model=model).qpos_fk(torch.from_numpy(g["qpos_euler"][:12].copy()))
    ball["qpos_quat"] = g["qpos_quat"][:12]
    beta = np.linspace(-1.0, 1.0, 16)

    def state(w, qpos):  # the world body in front of the 24 bodies of the record
        rows = lambda key, n: np.concatenate([np.eye(1, n), np.asarray(w[key][0]).reshape(-1, n)])
        return qpos, np.asarray(w["qvel"][0]), rows("wbpos", 3), rows("wbquat", 4), rows("body_com", 3)

    def length(is_ball, obs_v, has_shape, fut_frames=1, **v0):
        b, gender = (beta, 2.0) if has_shape else (None, None)
        if is_ball:
            qpos, qvel, xpos, xquat, _ = state(ball, ball["qpos_quat"][0])
            return len(E.full_obs_v2_quat(qpos, qvel, xpos, xquat, ball, 0, 0, b, gender))
        qpos, qvel, xpos, xquat, xipos = state(hinge, np.asarray(hinge["qpos"][0]))
        if obs_v == 1:  # (the oracle's v1 has no shape argument: humanoid_im.py:1390-1406 appends beta(16) + gender behind whichever version was computed)
            return len(E.full_obs_v1(qpos, qvel, xpos, xquat, xipos, hinge, 0, 0)) + (17 if has_shape else 0)
        if obs_v == 3:
            return len(E.full_obs_v3(qpos, qvel, xpos, xquat, hinge, 0, 0, b, gender, fut_frames=fut_frames, skip=4))
        if obs_v == 6:
            return len(E.full_obs_v6(qpos, qvel, xpos, hinge, 0, 0, b, gender))
        if obs_v == 5:
            return len(E.full_obs_v5(qpos, qvel, xpos, xquat, hinge, 0, 0, b, gender))
        if obs_v == 0:
            return len(E.full_obs_v0(qpos, qvel, hinge, 0, 0, **v0))
        if obs_v == 4:
            return len(E.full_obs_v4(qpos, qvel, xpos, xquat, hinge, 0, 0, b, gender)[0])
        return len(E.full_obs_v2(qpos, qvel, xpos, xquat, hinge, 0, 0, b, gender))

    return length


def test_the_dims_are_the_projects_models(model):
    from uhc_amd.model.mjcf import ball_variant
    from uhc_amd.sim import make_ctrl
    b = ball_variant(model)
    assert (model.nq, model.nv, model.nu, model.nbody, make_ctrl(model).action_dim) == tuple(HINGE[k] for k in ("nq", "nv", "nu", "nbody", "action_dim"))
    assert (b.nq, b.nv, b.nu, b.nbody) == tuple(BALL[k] for k in ("nq", "nv", "nu", "nbody"))


# what the GPU tests assert on the device (test_gpu_env.py, test_gpu_env_objects.py): obs_v, has_shape -> obs_dim, with their flags (v0: heading and phase; v3: 3 frames)
DEVICE_LITERALS = {(2, True): 657, (1, False): 784, (6, True): 401, (3, True): 3 * 657, (5, True): 653, (0, True): 220, (4, True): 643}


@pytest.mark.parametrize("objects", [0, 2])
@pytest.mark.parametrize("has_shape", [False, True])
@pytest.mark.parametrize("obs_v", range(7))
def test_obs_dim_of_every_version_on_the_hinge_humanoid(probe, oracle_len, model, obs_v, has_shape, objects):
    dims = with_objects(HINGE, objects) if objects else HINGE
    p, err = probe(dims, env_desc(model, obs_v=obs_v, has_shape=has_shape, fut_frames=3, fut_skip=4, obs_heading=True, root_deheading=True, obs_phase=True, num_obj=objects))
    assert err is None
    if (obs_v, has_shape) in DEVICE_LITERALS:
        assert p["obs_dim"] == DEVICE_LITERALS[(obs_v, has_shape)]
    assert p["obs_dim"] == oracle_len(False, obs_v, has_shape and obs_v != 0, fut_frames=3, obs_heading=True, root_deheading=True, obs_phase=True)
    # num_obj leaves the observation alone: the humanoid's extents are what is in front of the objects
    assert (p["n_obj"], p["nqh"], p["nvh"], p["nbh"], p["ball"]) == (objects, 76, 75, 25, 0)
    assert (p["nq"], p["nv"], p["nbody"]) == (76 + 7 * objects, 75 + 6 * objects, 25 + objects)
    assert p["has_shape"] == (int(has_shape) if obs_v != 0 else 0)  # get_full_obs never appends the shape
    assert (p["fut_frames"], p["fut_skip"]) == ((3, 4) if obs_v == 3 else (1, 0))


@pytest.mark.parametrize("obs_vel", ["full", "root"])
@pytest.mark.parametrize("phase", [False, True])
@pytest.mark.parametrize("heading", [False, True])
def test_obs_dim_of_v0_follows_its_flags(probe, oracle_len, model, heading, phase, obs_vel):
    p, err = probe(HINGE, env_desc(model, obs_v=0, has_shape=True, obs_heading=heading, root_deheading=True, obs_phase=phase, obs_vel=obs_vel))
    assert err is None
    assert p["obs_dim"] == oracle_len(False, 0, False, obs_heading=heading, root_deheading=True, obs_phase=phase, obs_vel=obs_vel)
    assert p["obs_dim"] == int(heading) + 74 + (6 if obs_vel == "root" else 75) + 69 + int(phase)
    assert p["obs_flags"] == int(heading) | 2 | int(phase) << 2 | int(obs_vel == "root") << 3


@pytest.mark.parametrize("fut_frames", [1, 3, 64])
def test_obs_dim_of_v3_is_fut_frames_of_v2(probe, oracle_len, model, fut_frames):
    p, err = probe(HINGE, env_desc(model, obs_v=3, has_shape=True, fut_frames=fut_frames, fut_skip=4))
    assert err is None
    assert p["obs_dim"] == fut_frames * 657 == oracle_len(False, 3, True, fut_frames=fut_frames)
    assert (p["fut_frames"], p["fut_skip"]) == (fut_frames, 4)


@pytest.mark.parametrize("objects", [0, 2])
@pytest.mark.parametrize("has_shape", [False, True])
def test_obs_dim_of_the_ball_humanoid(probe, oracle_len, model, has_shape, objects):
    dims = with_objects(BALL, objects) if objects else BALL
    p, err = probe(dims, env_desc(model, obs_v=2, has_shape=has_shape, num_obj=objects))
    assert err is None
    assert p["obs_dim"] == (534 if has_shape else 517) == oracle_len(True, 2, has_shape)
    assert (p["n_obj"], p["nqh"], p["nvh"], p["nbh"], p["ball"]) == (objects, 99, 75, 25, 1)


def test_the_plan_copies_the_batch_and_the_descriptor(probe, model):
    w = dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=2.0, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)
    d = env_desc(model, obs_v=2, reward_v=1, env_episode_len=321, env_expert_trail_steps=7, body_diff_thresh=0.25, reward_weights=w, env_term_body="root")
    p, err = probe(dict(HINGE, n_env=5, action_dim=81, vf_dim=216), d)
    assert err is None
    assert (p["n_env"], p["nu"], p["action_dim"], p["vf_dim"]) == (5, 69, 81, 216)
    assert (p["obs_v"], p["reward_v"], p["term_body"], p["env_episode_len"], p["expert_trail_steps"]) == (2, 1, 1, 321, 7)
    assert [p[f"ee{k}"] for k in range(5)] == list(d.ee_body)
    assert p["doubles"] == [1.0 / 30, 0.25] + list(d.reward_weights) + [0.7071, -0.7071, 0.0, 0.0]


def refusal(probe, model, dims=HINGE, **fields):
    d = env_desc(model)
    for k, v in fields.items():
        setattr(d, k, v)
    return probe(dims, d)[1]


REFUSED = [  # (what, dims, descriptor fields, the text uhc_env_create has always given)
    ("obs_v -1", HINGE, dict(obs_v=-1), OBS_V_TEXT),
    ("obs_v 7", HINGE, dict(obs_v=7), OBS_V_TEXT),
    ("v3, fut_frames 0", HINGE, dict(obs_v=3, fut_frames=0), FUT_TEXT),
    ("v3, fut_frames 65", HINGE, dict(obs_v=3, fut_frames=65), FUT_TEXT),
    ("v3, fut_skip -1", HINGE, dict(obs_v=3, fut_skip=-1), FUT_TEXT),
    ("term_body 2", HINGE, dict(term_body=2), TERM_TEXT),
    ("reward_v -1", HINGE, dict(reward_v=-1), REWARD_V_TEXT),
    ("reward_v 6", HINGE, dict(reward_v=6), REWARD_V_TEXT),
    ("num_obj -1", with_objects(HINGE), dict(num_obj=-1), NUM_OBJ_TEXT),
    ("num_obj 1, no free body", HINGE, dict(num_obj=1), NUM_OBJ_TEXT),
    ("num_obj 3, two free bodies", with_objects(HINGE), dict(num_obj=3), NUM_OBJ_TEXT),
    ("num_obj 3, two free bodies, ball", with_objects(BALL), dict(num_obj=3), NUM_OBJ_TEXT),
    ("nq 193", dict(HINGE, nq=193, nv=192), {}, DIMS_TEXT),
    ("65 non-root bodies", dict(HINGE, nbody=66), {}, DIMS_TEXT),
    ("no non-root body", dict(HINGE, nbody=1), {}, DIMS_TEXT),
    ("neither hinge nor ball", dict(HINGE, nq=80), {}, DIMS_TEXT),
    ("two objects claimed as humanoid", with_objects(HINGE), {}, DIMS_TEXT),
    ("ball, obs_v 1", BALL, dict(obs_v=1), BALL_TEXT),
    ("ball, reward_v 1", BALL, dict(reward_v=1), BALL_TEXT),
    ("ball with objects, obs_v 6", with_objects(BALL), dict(obs_v=6, num_obj=2), BALL_TEXT),
]


@pytest.mark.parametrize("what,dims,fields,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_refusal_keeps_its_text(probe, model, what, dims, fields, text):
    assert refusal(probe, model, dims, **fields) == text


ACCEPTED = [
    ("v3, fut_frames 1", HINGE, dict(obs_v=3, fut_frames=1, fut_skip=0)),
    ("v3, fut_frames 64", HINGE, dict(obs_v=3, fut_frames=64)),
    ("fut_frames 0 outside v3", HINGE, dict(obs_v=2, fut_frames=0, fut_skip=-1)),
    ("nq 192", dict(HINGE, nq=192, nv=191), {}),
    ("64 non-root bodies", dict(HINGE, nbody=65), {}),
    ("num_obj = the trailing free bodies", with_objects(HINGE), dict(num_obj=2)),
    ("num_obj below the trailing free bodies", with_objects(HINGE, 1) | dict(n_trailing_free=2), dict(num_obj=1)),
    ("reward_v 5, term_body 1", HINGE, dict(reward_v=5, term_body=1)),
]


@pytest.mark.parametrize("what,dims,fields", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_the_accepted_neighbours_are_accepted(probe, model, what, dims, fields):
    assert refusal(probe, model, dims, **fields) is None


def test_a_descriptor_with_two_faults_reports_the_first(probe, model):
    assert refusal(probe, model, obs_v=7, reward_v=9) == OBS_V_TEXT
    assert refusal(probe, model, obs_v=3, fut_frames=0, term_body=2) == FUT_TEXT
    assert refusal(probe, model, term_body=2, reward_v=9) == TERM_TEXT
    assert refusal(probe, model, reward_v=9, num_obj=1) == REWARD_V_TEXT
    assert refusal(probe, model, dict(HINGE, nq=80), num_obj=1) == NUM_OBJ_TEXT
    assert refusal(probe, model, dict(BALL, nq=193, nv=192), obs_v=1) == DIMS_TEXT
