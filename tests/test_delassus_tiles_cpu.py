"""The Delassus build's index maps (uhc_amd/csrc/uhc_delassus_tiles.h) without a GPU: tests/delassus_tiles_probe.cpp, a stand-alone program built with the
host compiler, emulates the 16 x 16 x 4 matrix instruction from the lane maps and runs gather -> tiles -> transposition as k_pgs_fast does -- on a chain of 32
dofs, random trees of 1 / 6 / 75 / 99 / 128 dofs, the shipped humanoid's tree and its ball-joint variant's, at every row count on both sides of a tile edge, with
dense rows in lane 0 and in the last lane -- against the naive double loop over the common chain prefix; and the chain-position masks against the chains
themselves for every (dof, ancestor) pair."""
import subprocess

import pytest

from tests import probe_build

NEFC = (1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64)
BUILTIN_TREES = 6


def build_probe(tag, extra=()):
    return probe_build.build_probe("delassus_tiles_probe" + tag, ["tests/delassus_tiles_probe.cpp"], ["uhc_amd/csrc/uhc_delassus_tiles.h"], ("-Wall", "-Werror", *extra))


@pytest.fixture(scope="module")
def tree_files(tmp_path_factory):
    """the dof trees of the shipped model, of its ball-joint variant and of that variant among four free boxes, as the probe reads them"""
    from tests.test_batch_plan_cpu import model_class
    base, ball, boxes = (model_class(n)[0] for n in ("asset", "ball", "ball_boxes"))
    d = tmp_path_factory.mktemp("trees")
    files = []
    for name, m in (("humanoid", base), ("ball", ball), ("ball_boxes", boxes)):
        p = d / (name + ".txt")
        p.write_text(f"{name} {m.nv}\n" + " ".join(str(int(x)) for x in m.dof_parentid) + "\n")
        files.append(str(p))
    assert base.nv == 75 and ball.nv == 75 and ball.nq == 99 and boxes.nv == 99  # (the boxes' free joints: dofs in both words of the masks)
    return files


def check(exe, tree_files):
    r = subprocess.run([exe] + tree_files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == BUILTIN_TREES + len(tree_files) + 1 and all(l.startswith("tree ") for l in lines[:-1]), r.stdout
    assert [l.split()[1] for l in lines[BUILTIN_TREES:-1]] == ["humanoid", "ball", "ball_boxes"]
    # per tree: every row count x (0, 2, 5 dense rows) x two draws
    assert lines[-1] == f"OK {(BUILTIN_TREES + len(tree_files)) * len(NEFC) * 3 * 2}", lines[-1]


def test_maps_gather_tiles_and_transposition_match_the_naive_build(tree_files):
    check(build_probe(""), tree_files)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(tree_files):
    """the probe as a stand-alone program of its own, every index it forms checked"""
    check(build_probe("_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")), tree_files)


@pytest.mark.parametrize("name", ["asset", "ball", "ball_boxes", "chain32"])
def test_the_planners_chain_masks_are_the_planners_chains(name):
    """BatchPlan::chainmask -- what uhc_batch_create uploads as DevTopo::dof_chainmask, [nv][2] words -- against the same plan's dof_anc: for every dof and every
    position q on its chain, the ancestor's bit is set and the number of set bits below it is q; no other bit is set."""
    import ctypes as C

    import numpy as np

    from tests.test_batch_plan_cpu import Probe, model_class
    so = probe_build.build_probe("chainmask_probe.so", ["tests/chainmask_probe.cpp", "uhc_amd/csrc/uhc_plan.cpp"],
                                 ["tests/plan_probe.cpp"] + ["uhc_amd/csrc/" + h for h in ("uhc_plan.h", "uhc_host.h", "uhc_device.h", "uhc_step_words.h", "uhc_delassus_tiles.h")],
                                 probe_build.HIP_STRUCT_FLAGS)
    p = Probe(so)
    m, ctrl = model_class(name)
    words, _ = p.plan(m, ctrl, 64)
    nv, ys = words["t.nv"], words["t.maxdepth"] + 1
    anc = p.table("dof_anc", np.int16).reshape(nv, ys)
    depth = p.table("dof_depth", np.int32)
    p.L.uhc_plan_probe_chainmask.restype = C.c_longlong
    buf = (C.c_ulonglong * (2 * nv))()
    assert p.L.uhc_plan_probe_chainmask(buf, 2 * nv) == 2 * nv
    for i in range(nv):
        mask = int(buf[2 * i]) | (int(buf[2 * i + 1]) << 64)
        chain = [int(anc[i, q]) for q in range(depth[i] + 1)]
        assert chain[-1] == i and mask == sum(1 << a for a in chain), (i, chain, hex(mask))
        for q, a in enumerate(chain):
            assert bin(mask & ((1 << a) - 1)).count("1") == q, (i, q, a)
