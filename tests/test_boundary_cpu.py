"""CPU: the reference's import surface resolves (the `uhc` alias package), with the reference's registry keys and call signatures."""
import inspect


def test_reference_import_paths_resolve_to_this_build():
    import uhc_amd.agents
    import uhc_amd.agents.agent_copycat as real
    from uhc.agents import agent_dict                     # scripts/train_uhc.py:32
    from uhc.agents.agent_copycat import AgentCopycat     # scripts/train_uhc.py:90
    from uhc.data_loaders.dataset_amass_single import DatasetAMASSSingle
    from uhc.envs import env_dict
    from uhc.khrylib.rl.core import PolicyGaussian, Value, estimate_advantages  # noqa: F401
    from uhc.khrylib.utils.zfilter import ZFilter  # noqa: F401
    from uhc.smpllib.smpl_mujoco import SMPLConverter, smpl_to_qpose  # noqa: F401
    from uhc.utils.config_utils.copycat_config import Config  # scripts/train_uhc.py:31
    from uhc.utils.flags import flags  # noqa: F401
    assert agent_dict is uhc_amd.agents.agent_dict and AgentCopycat is real.AgentCopycat
    assert set(agent_dict) == {"agent_copycat"} and set(env_dict) == {"humanoid_im"}
    # constructor / method signatures the reference's callers rely on (agent_copycat.py:55, humanoid_im.py:49, dataset_amass_single.py)
    assert list(inspect.signature(AgentCopycat.__init__).parameters)[:6] == ["self", "cfg", "dtype", "device", "training", "checkpoint_epoch"]
    assert list(inspect.signature(env_dict["humanoid_im"].__init__).parameters)[:6] == ["self", "cfg", "init_expert", "data_specs", "mode", "no_root"]
    assert list(inspect.signature(DatasetAMASSSingle.sample_seq).parameters)[:6] == ["self", "full_sample", "freq_dict", "sampling_temp", "sampling_freq", "precision_mode"]
    for name in ("reset", "step", "load_expert", "set_mode", "seed", "get_expert_attr", "get_expert_index", "get_wbody_pos", "get_world_vf", "fail_safe",
                 "get_ee_pos", "get_body_quat", "get_com", "get_humanoid_qpos"):
        assert callable(getattr(env_dict["humanoid_im"], name)), name
    assert Config.__module__ == "uhc_amd.utils.config_utils.copycat_config"
    import pytest
    with pytest.raises(ModuleNotFoundError):
        import uhc.no_such_module  # noqa: F401


def _load_bench(path, name):
    """bench.py as a module, with this process's environment as it was: bench.py sets OMP_PROC_BIND / OMP_PLACES defaults at import, and a bench
    subprocess started later by another test would inherit them and have its OpenMP runtime bind the main thread to one core at `import torch`."""
    import importlib.util
    import os
    env = dict(os.environ)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        bench = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bench)
    finally:
        os.environ.clear()
        os.environ.update(env)
    return bench


def test_bench_defaults_are_the_drivers_contract():
    """`python bench.py` with no flags: one GPU, a step count that finishes in minutes, the metric's configuration (1 024 envs, exact
    contact solve, float64 learner); the flags the driver passes exist."""
    import os
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = _load_bench(os.path.join(ROOT, "bench.py"), "bench_cli")
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    assert a.gpus == 1 and a.steps == 50 and a.warmup == 10 and a.envs == 1024 and a.workload == "copycat" and a.ppo_dtype == "float64"
    assert a.solver is None and not a.general_only and not a.fixed_path and a.shapes == 0
    sys.argv = ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"]
    try:
        b = bench.parse()
    finally:
        sys.argv = argv
    assert (b.gpus, b.steps, b.warmup) == (8, 20, 5)


def test_bench_plain_run_leaves_the_extras_to_full(tmp_path):
    """A plain run measures the headline only; --full brings back the PPO update, the PGS timings, the probes and the CPU baselines (each still
    behind its --no-* switch).  --dump-outputs keeps to its size cap with the same seeded rows of every array, listed in env_ids.npy."""
    import os
    import sys
    import numpy as np
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = _load_bench(os.path.join(ROOT, "bench.py"), "bench_cli3")
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
        a = bench.parse()
        sys.argv = ["bench.py", "--full", "--no-ppo"]
        b = bench.parse()
    finally:
        sys.argv = argv
    assert not a.full and a.no_ppo and a.no_pgs_probe and a.no_probes and a.no_cpu_baseline and a.dump_outputs is None
    assert b.full and b.no_ppo and not b.no_pgs_probe and not b.no_probes and not b.no_cpu_baseline
    x = np.arange(4000.0).reshape(1000, 4)
    y = np.ones((1000, 2), dtype=np.float32)
    bench.DUMP_LIMIT = 20000
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), {"x": x, "y": y})
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["env_ids.npy", "x.npy", "y.npy"] and all(v.dtype == np.float64 for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in got) <= 20000
    ids = got["env_ids.npy"].astype(int)
    assert len(ids) > 100 and (np.diff(ids) > 0).all()
    np.testing.assert_array_equal(got["x.npy"], x[ids])
    for f in got:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f), got[f])
    bench.DUMP_LIMIT = 64 << 20
    bench.dump_outputs(str(tmp_path / "c"), {"x": x})
    assert sorted(os.listdir(tmp_path / "c")) == ["x.npy"] and np.array_equal(np.load(tmp_path / "c" / "x.npy"), x)


def test_bench_reads_every_committed_profile():
    """bench.py quotes two numbers from the committed profiles (contact-solve share of the stage profile, float64 VALU counters of the PMC
    pass); whatever a measurement pass leaves under profiles/ must parse -- a profile format change may not break the bench line."""
    import glob
    import os
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = _load_bench(os.path.join(ROOT, "bench.py"), "bench_cli2")
    share, src = bench.contact_solve_share()
    assert src and 0.02 < share < 0.6
    c = bench.valu_f64_counters(bench.FAST_KERNEL[False])
    assert c and c["flop_per_launch"] > 1e9
    t, tsrc = bench.pmc_traffic(bench.FAST_KERNEL[False])
    ms, msrc = bench.rocprof_avg_ms(bench.FAST_KERNEL[True], "_selfcol")  # the kernel trace of the headline workload, quoted beside the HIP-event time
    assert msrc and 1.0 < ms < 50.0 and bench.rocprof_avg_ms("no such kernel") == (None, None)
    assert tsrc and t > 1e6
    for name in ("headline", "floor_only", "shapes", "configs4", "ball_rollout"):  # per-workload counter passes (tools/pmc_alu.py), where committed
        a = bench.alu_per_env_step(name)
        assert a is None or (a["flop_per_env_step"] > 1e6 and a["source"].endswith(".json")), name
    # the probe at configs[2]'s batch size is the headline's workload: it is priced with the headline's flop per env-step
    assert (bench.alu_per_env_step("configs2_per_gpu") or {}).get("source") == (bench.alu_per_env_step("headline") or {}).get("source")
    # every BASELINE config that fits one GPU has a probe, and the probe of configs[2] runs at its 4096 envs per GPU
    assert set(bench.PROBES) == {"configs2_per_gpu", "floor_only", "shapes", "ball_rollout", "configs4"} and bench.PROBES["configs2_per_gpu"]["envs"] == 4096
    assert bench.PROBES["configs4"]["objects"] == 4 and bench.PROBES["configs4"]["robot_cfg"]["ball"] and bench.PROBES["ball_rollout"]["robot_cfg"]["ball"]
    r = bench.step_roofline("no_such_workload", 1024, 1e5, 3.5, 76, 75, 25, 105)
    assert r["bound"] == "fp64_valu" and r["achieved"] is None and r["hbm"]["achieved_GBs"] > 0
    latest, bench._latest = bench._latest, None
    try:  # ... and every older file of the same kinds, not only the latest
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_stage_profile.txt"))):
            bench._latest = lambda pattern, f=f: f
            s, _ = bench.contact_solve_share()
            assert s is None or 0.02 < s < 0.6, f
    finally:
        bench._latest = latest


def test_every_uhc_import_line_of_the_references_agent_and_env_resolves():
    """uhc/agents/agent_copycat.py:31-48 and the header of uhc/envs/humanoid_im.py:14-44, line by line (VERDICT r4 missing 5): a maintainer who
    keeps the reference's agent_copycat.py imports it against this build.  The file-level paths of packages this build keeps in one module
    resolve through the alias finder's table (uhc/__init__.py `_SPLIT`) to the module that defines the names."""
    lines = """
from uhc.khrylib.utils import to_device, create_logger, ZFilter, get_eta_str
from uhc.khrylib.rl.core import LoggerRL
from uhc.khrylib.utils.memory import Memory
from uhc.khrylib.utils.torch import *
from uhc.khrylib.rl.core import estimate_advantages
from uhc.khrylib.rl.agents import AgentPPO
from uhc.khrylib.rl.core.policy_gaussian import PolicyGaussian
from uhc.khrylib.rl.core.critic import Value
from uhc.losses.reward_function import reward_func
from uhc.models.policy_mcp import PolicyMCP
from uhc.khrylib.models.mlp import MLP
from uhc.envs.humanoid_im import HumanoidEnv
from uhc.data_loaders.dataset_amass_single import DatasetAMASSSingle
from uhc.smpllib.smpl_parser import SMPL_BONE_ORDER_NAMES
from uhc.smpllib.smpl_eval import compute_metrics
from uhc.utils.flags import flags
from uhc.utils.tools import CustomUnpickler
from uhc.utils.torch_utils import quaternion_matrix_batch
from uhc.utils.tools import get_expert, get_expert_master
from uhc.khrylib.utils.transformation import quaternion_from_euler
from uhc.khrylib.utils import *
from uhc.khrylib.rl.envs.common import mujoco_env
from uhc.utils.transformation import (quaternion_from_euler_batch, quaternion_multiply_batch, quat_mul_vec, quat_mul_vec_batch, quaternion_from_euler, quaternion_inverse_batch)
from uhc.utils.math_utils import *
from uhc.smpllib.smpl_mujoco import SMPLConverter
from uhc.smpllib.torch_smpl_humanoid import Humanoid
from uhc.smpllib.smpl_robot import Robot, in_hull
from uhc.smpllib.smpl_mujoco import smpl_6d_to_qpose, smpl_to_qpose, qpos_to_smpl
from uhc.smpllib.smpl_parser import (SMPL_EE_NAMES, SMPL_BONE_ORDER_NAMES, SMPLH_BONE_ORDER_NAMES)
from uhc.khrylib.rl.core.common import estimate_advantages
from uhc.khrylib.rl.core.trajbatch import TrajBatch
from uhc.khrylib.rl.core.logger_rl import LoggerRL
from uhc.khrylib.rl.agents.agent_ppo import AgentPPO
""".strip().splitlines()
    ns = {}
    for ln in lines:
        exec(ln, ns)  # noqa: S102  (the point of the test: the reference's own import statements)
    import uhc_amd.khrylib.rl.core as core
    import uhc_amd.utils.tools as tools
    assert ns["PolicyGaussian"] is core.PolicyGaussian and ns["Value"] is core.Value and ns["CustomUnpickler"] is tools.CustomUnpickler
    assert issubclass(ns["HumanoidEnv"], ns["mujoco_env"].MujocoEnv)
    assert len(ns["SMPLH_BONE_ORDER_NAMES"]) == 52 and ns["SMPLH_BONE_ORDER_NAMES"][22] == "L_Index1" and ns["SMPLH_BONE_ORDER_NAMES"][-1] == "R_Thumb3"
    import uhc_amd.agents.agent_copycat as ac
    assert ac.CustomUnpickler is tools.CustomUnpickler  # (its old home re-exports it)


def test_memory_and_trajbatch_keep_the_references_field_order():
    """uhc/khrylib/utils/memory.py:4-23, uhc/khrylib/rl/core/trajbatch.py:5-15: workers push (state, action, mask, next_state, reward, exp)
    tuples, TrajBatch merges the workers' memories in list order and stacks each field."""
    import numpy as np
    from uhc.khrylib.rl.core.trajbatch import TrajBatch
    from uhc.khrylib.utils.memory import Memory
    rng = np.random.default_rng(0)
    mems, rows = [], []
    for w in range(3):
        m = Memory()
        for t in range(4 + w):
            row = (rng.normal(size=5), rng.normal(size=2), float(t % 2), rng.normal(size=5), float(rng.normal()), 1.0 - (t % 3 == 0))
            m.push(*row)
            rows.append(row)
        mems.append(m)
    assert [len(m) for m in mems] == [4, 5, 6] and len(mems[0].sample(2)) == 2
    b = TrajBatch(mems)
    assert b.states.shape == (15, 5) and b.actions.shape == (15, 2) and b.masks.shape == (15,) and b.exps.shape == (15,)
    for k, name in enumerate(TrajBatch.FIELDS):
        np.testing.assert_array_equal(getattr(b, name), np.stack([r[k] for r in rows]))


def test_pose_converters_invert_each_other(model):
    """qpos_to_smpl (smpl_mujoco.py:738-752) inverts smpl_to_qpose; smpl_6d_to_qpose (:776-780) of the 6D rotations process_amass_db writes equals
    smpl_to_qpose of the axis-angle pose they came from (to the float32 of the 6D encoding); in_hull (smpl_robot.py:73-80) on a cube."""
    import numpy as np
    from scipy.spatial import ConvexHull
    from scipy.spatial.transform import Rotation as sRot
    from uhc.data_process.process_amass_db import convert_aa_to_orth6d
    from uhc.smpllib.smpl_mujoco import qpos_to_smpl, smpl_6d_to_qpose, smpl_to_qpose
    from uhc.smpllib.smpl_robot import in_hull
    rng = np.random.default_rng(3)
    pose = rng.normal(scale=0.4, size=(6, 72))
    trans = rng.normal(size=(6, 3))
    qpos = smpl_to_qpose(pose, model, trans=trans.copy())
    back, tback = qpos_to_smpl(qpos, model)
    np.testing.assert_allclose(tback, trans, atol=1e-12)
    for a, b in zip(back.reshape(-1, 3), pose.reshape(-1, 3)):  # same rotation (rotation vectors are unique below pi)
        np.testing.assert_allclose(sRot.from_rotvec(a).as_matrix(), sRot.from_rotvec(b).as_matrix(), atol=1e-9)
    full = np.concatenate([trans, convert_aa_to_orth6d(pose).reshape(6, -1)], axis=1)
    np.testing.assert_allclose(smpl_6d_to_qpose(full, model), qpos, atol=2e-6)
    cube = ConvexHull(np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=float))
    assert in_hull(cube, np.array([[0, 0, 0], [0.9995, 0, 0], [1.0005, 0, 0], [1.01, 0, 0]])).tolist() == [True, True, True, False]
    assert in_hull(cube, np.array([0.5, 0.5, 0.5])).tolist() == [True]
