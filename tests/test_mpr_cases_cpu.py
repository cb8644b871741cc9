"""The oracle's convex narrow phase (oracle/physics_oracle.c: mpr_penetration, a restatement of libccd's MPR that no MuJoCo pins in this image) against plain geometry, on
the case table of tests/mpr_cases.py -- the inputs tests/test_gpu_mpr_edges.py then holds the device to.  "Device equals oracle" is worth what the oracle is worth.

Per hull family the file prints the number of cases, hits and misses, the share in MPR's tolerance band, the share whose answer is discontinuous, and the largest
depth - h(n).  Arithmetic is long double where a comparison is tight."""
import numpy as np
import pytest

from tests import mpr_cases as M

LD = np.longdouble


def _hulls(name, e):
    m = M.family_model(name)
    q, _, _ = M.family_cases(name)
    return M.world_hull(m, 1, q[e, :3], q[e, 3:7]), M.world_hull(m, 2, q[e, 7:10], q[e, 10:14])


@pytest.mark.parametrize("name", list(M.FAMILIES))
def test_oracle_contacts_agree_with_the_polytopes_geometry(name):
    """A contact where the polytopes are at most margin - 1e-5 apart, none where they are at least margin + 1e-6 apart (between the two lies MPR's tolerance: not judged, and
    at most 5 % of the table); on every contact depth <= h(n) + 1e-12 (no penetration along n is deeper than the Minkowski difference's extent along n -- the converse does not
    hold: the closest point of the last portal triangle may lie on its edge), |n| = 1, n from geom 1 to geom 2, the point inside the box of the midpoints (a + b) / 2."""
    m = M.family_model(name)
    assert (int(m.geom_vertnum[1]), int(m.geom_vertnum[2])) == M.VERTS[name]  # the compiler kept the hulls as given
    q, _, tags = M.family_cases(name)
    ref = M.family_reference(name)
    assert set(tags) == set(M.TAGS)
    hits = misses = band = 0
    worst = -np.inf
    for e in range(len(q)):
        (A, ra, ca), (B, rb, cb) = _hulls(name, e)
        lo, hi = M.polytope_distance(A, B)
        lo, hi = lo - ra - rb, hi - ra - rb
        r = ref[e]
        assert r["ncon"] in (0, 1) and r["fail"] == 0
        if hi <= M.MARGIN - 1e-5:
            assert r["ncon"] == 1, (name, e, tags[e], lo, hi)
        elif lo >= M.MARGIN + 1e-6:
            assert r["ncon"] == 0, (name, e, tags[e], lo, hi)
        else:
            band += 1
        hits += r["ncon"]
        misses += 1 - r["ncon"]
        if not r["ncon"]:
            continue
        n, pos, depth = r["normal"][0], r["pos"][0], LD(M.MARGIN) - LD(r["dist"][0])
        over = float(depth - LD(M.support_depth_bound(A, ra, B, rb, n)))
        worst = max(worst, over)
        assert over <= 1e-12, (name, e, tags[e], over)
        assert abs(float(np.sqrt((n.astype(LD) ** 2).sum())) - 1.0) <= 4e-16, (name, e)
        if np.abs(cb - ca).max() > 1e-12:
            assert n @ (cb - ca) > 0, (name, e, tags[e])
        # (a + b) / 2 over the inflated hulls: within the box of the vertex midpoints, grown by the half-margins and radii
        grow = 0.5 * (ra + rb + M.MARGIN) + 1e-12
        mid_lo, mid_hi = 0.5 * (A.min(axis=0) + B.min(axis=0)) - grow, 0.5 * (A.max(axis=0) + B.max(axis=0)) + grow
        assert (pos >= mid_lo).all() and (pos <= mid_hi).all(), (name, e, tags[e], pos)
    spread, _ = M.family_spread(name)
    jumpy = int((spread > M.SPREAD_BAR).sum())
    print(f"MPR CASES {name:16s} vertices {M.VERTS[name]}: {len(q)} cases, {hits} hits, {misses} misses, in the tolerance band {band} ({100.0 * band / len(q):.1f} %), "
          f"discontinuous {jumpy} ({100.0 * jumpy / len(q):.1f} %: {[tags[e] for e in np.nonzero(spread > M.SPREAD_BAR)[0]]}), largest depth - h(n) {worst:.2e}")
    assert band <= 0.05 * len(q), (name, band)
    assert hits >= 10 and misses >= 10, (name, hits, misses)


def test_the_tables_discontinuous_share_is_at_most_two_percent():
    """The oracle against itself 1e-15 away (tests/mpr_cases.py: perturbations): a case whose qacc moves by more than 1e-8 is a discontinuity of the contact model, which the
    GPU file may judge by the oracle's branches only.  At most 2 % of the table, for the forward pass and for the stepped form the queue consumers are held to."""
    for stepped in (False, True):
        total = jumpy = 0
        worst_stable = 0.0
        for name in M.FAMILIES:
            spread, _ = M.family_spread(name, stepped)
            total += len(spread)
            jumpy += int((spread > M.SPREAD_BAR).sum())
            worst_stable = max(worst_stable, float(spread[spread <= M.SPREAD_BAR].max()))
        print(f"MPR CASES {'stepped' if stepped else 'forward'}: {jumpy} of {total} cases discontinuous ({100.0 * jumpy / total:.2f} %); the others move by at most {worst_stable:.2e}")
        assert jumpy <= 0.02 * total, (stepped, jumpy, total)


def test_coincident_centres_take_the_eps_branch():
    """The coincident cases are coincident to the device too: the centres, computed as the kernels do (R c + x), differ by less than libccd's epsilon in every coordinate."""
    from uhc_amd.model.mjcf import quat_to_mat
    for name in M.FAMILIES:
        m = M.family_model(name)
        q, _, tags = M.family_cases(name)
        for e in [k for k, t in enumerate(tags) if t == "coincident"]:
            c = [quat_to_mat(q[e, 7 * k + 3:7 * k + 7]) @ np.asarray(m.geom_center[k + 1]) + q[e, 7 * k:7 * k + 3] for k in range(2)]
            assert np.abs(c[0] - c[1]).max() < 2.220446049250313e-16, (name, e, c)
            assert np.abs(np.asarray(m.geom_center[1:3])).max() < 1e-16  # (so small that rounding and contraction of R c + x cannot matter)


@pytest.mark.parametrize("u", [np.array([1.0, 0, 0]), np.array([0.0, 0.6, 0.8]), M.POLE], ids=["x", "yz", "pole"])
def test_poles_ball_along_three_directions(u):
    """The balls with exact poles, turned so that their poles lie along u and overlapping by d along it: the first support point lies on the centre line (the origin on the
    segment v0 - v1), depth d + margin to 2e-6, normal u to 1e-6, the point on the centre line in the middle of the lens."""
    from oracle.physics import OracleSim
    m = M.family_model("poles")
    Rw = M._rot_to(M.POLE, u)
    ra, rb, d = 0.1, 0.07, 0.012
    ca = np.array([0.0, 0.0, M.HEIGHT])
    s = OracleSim(m)
    s.set_state(M.pose_q(ca, Rw, ca + (ra + rb - d) * u, Rw), np.zeros(12))
    assert s.geti("ncon") == 1
    assert s.get("con_dist")[0] == pytest.approx(-d, abs=2e-6)
    np.testing.assert_allclose(s.get("con_frame")[:3], u, atol=1e-6)
    np.testing.assert_allclose(s.get("con_pos")[:3], ca + (ra - d / 2) * u, atol=2e-6)


@pytest.mark.parametrize("name,reach", [("box_sphere", 0.05), ("box_capsule", 0.09)])
@pytest.mark.parametrize("gap", [-0.004, 0.0004])
def test_rounded_hull_over_a_box_face(name, reach, gap):
    """A sphere, and a capsule standing on its end, over the +z face of the box (off its middle): dist = gap to 2e-6, normal +z (from the box to the rounded hull) to 1e-6."""
    from oracle.physics import OracleSim
    from scipy.spatial.transform import Rotation as sR
    m = M.family_model(name)
    ca = np.array([0.0, 0.0, M.HEIGHT])
    Rb = sR.from_euler("y", -np.pi / 2)  # the capsule's axis (x) along z
    s = OracleSim(m)
    s.set_state(M.pose_q(ca, sR.identity(), ca + [0.013, -0.021, 0.1 + reach + gap], Rb), np.zeros(12))
    assert s.geti("ncon") == 1
    assert s.get("con_dist")[0] == pytest.approx(gap, abs=2e-6)
    np.testing.assert_allclose(s.get("con_frame")[:3], [0, 0, 1], atol=1e-6)


@pytest.mark.parametrize("name", list(M.FAMILIES))
def test_covariance_on_one_case_per_family(name):
    """test_mpr_is_rotation_and_translation_covariant's bars on the first stable random hit of every family: the same scene turned and moved gives the same depth (1e-6),
    the turned normal and the moved point (1e-5)."""
    from oracle.physics import OracleSim
    from scipy.spatial.transform import Rotation as sR
    m = M.family_model(name)
    q, _, tags = M.family_cases(name)
    ref = M.family_reference(name)
    spread, _ = M.family_spread(name)
    e = next(k for k in range(len(q)) if tags[k] == "random" and ref[k]["ncon"] == 1 and spread[k] <= M.SPREAD_BAR and ref[k]["dist"][0] < -1e-4)
    Rw, tw = sR.from_rotvec([0.3, -1.1, 0.5]), np.array([0.4, -0.2, 3.0])
    R = [sR.from_quat(np.roll(q[e, 7 * k + 3:7 * k + 7], -1)) for k in range(2)]
    s = OracleSim(m)
    s.set_state(M.pose_q(Rw.apply(q[e, :3]) + tw, Rw * R[0], Rw.apply(q[e, 7:10]) + tw, Rw * R[1]), np.zeros(12))
    assert s.geti("ncon") == 1
    assert s.get("con_dist")[0] == pytest.approx(ref[e]["dist"][0], abs=1e-6)
    np.testing.assert_allclose(s.get("con_frame")[:3], Rw.apply(ref[e]["normal"][0]), atol=1e-5)
    np.testing.assert_allclose(s.get("con_pos")[:3], Rw.apply(ref[e]["pos"][0]) + tw, atol=1e-5)


# ------------------------------------------------------------------ the scenes of more than two bodies
@pytest.mark.parametrize("name", ["three", "four"])
def test_small_scenes_have_hits_and_misses(name):
    m, q, v = M.multi_scene(name)
    ref = M.multi_reference(name)
    n = m.nbody - 1
    pairs = n * (n - 1) // 2
    ncon = np.array([r["ncon"] for r in ref])
    print(f"MPR CASES scene {name}: {pairs} pairs, contacts per env {ncon.tolist()}")
    assert ncon.max() == pairs and ncon.min() < pairs and all(r["fail"] == 0 for r in ref)  # every request count of a round from `pairs` down occurs in some env


@pytest.mark.parametrize("name", list(M.SCENES))
def test_rod_scenes_put_every_pair_past_the_bounding_spheres(name):
    """Every pair of rods passes the bounding-sphere test (so without the box cull every pair is a candidate: 66, 253 <= CAND_CAP, 276 > CAND_CAP) while only a handful of
    pairs are in contact: fewer than the fast tier's 12 body-body rows."""
    from uhc_amd.model.mjcf import kinematics_np, quat_to_mat
    n, joint, pairs = M.SCENES[name]
    m, q, v = M.multi_scene(name)
    assert m.nbody - 1 == n and n * (n - 1) // 2 == pairs and m.nv == (6 * n if joint == "free" else n)
    assert (pairs > M.CAND_CAP) == (name == "rods24")
    for e in range(len(q)):
        xp, xq, _, _ = kinematics_np(m, q[e])
        c = np.array([quat_to_mat(xq[b]) @ np.asarray(m.geom_center[b]) + xp[b] for b in range(1, n + 1)])  # (geom g sits on body g: the floor is geom 0 of the world)
        d = np.linalg.norm(c[:, None] - c[None], axis=2)
        assert (d < 2 * m.geom_rbound[1] + M.MARGIN - 1e-3).all(), d.max()
    ref = M.multi_reference(name)
    print(f"MPR CASES scene {name}: {pairs} pairs past the bounding spheres, contacts per env {[r['ncon'] for r in ref]}")
    assert all(2 <= r["ncon"] <= 8 and r["fail"] == 0 for r in ref)


# ------------------------------------------------------------------ what the plan does with these models
def _all_models():
    out = {name: M.family_model(name) for name in M.FAMILIES}
    out.update({name: M.multi_scene(name)[0] for name in ("three", "four", *M.SCENES)})
    return out


def test_plan_stages_every_model_and_keeps_256_candidate_slots():
    """Whether a tier reads the hull vertices from LDS or from global memory is the plan's decision (cp.vstage: the vertices must fit the region the dense rows will use).
    Every model of this table is staged by the fast, the general and the large tier, so the LDS form of mpr_wave is what an unset UHC_DEBUG runs and DEBUG_NO_VSTAGE is
    what reaches the global form, on every model.  And the candidate list: CAND_CAP = 256 ints on rowMisc, whose region holds at least 128 doubles in every tier."""
    from tests.helpers import passive_ctrl
    from tests.test_batch_plan_cpu import Probe, _regions, build_probe
    from uhc_amd.sim import DEBUG_NO_VSTAGE
    P = Probe(build_probe())
    for name, m in _all_models().items():
        W, _ = P.plan(m, passive_ctrl(m), 64)
        W0, _ = P.plan(m, passive_ctrl(m), 64, f"UHC_DEBUG={DEBUG_NO_VSTAGE}")
        staged = [W[c + "vstage"] >= 0 for c in ("cf.", "cg.", "ch.")]
        print(f"MPR CASES plan {name:16s} {3 * W['t.nmeshvert']:5d} doubles of vertices, {W['t.ncpair']:3d} pairs: staged by fast / general / large {staged}, by tier 4 {W['cx.vstage'] >= 0}")
        assert W["t.ncpair"] == (m.nbody - 1) * (m.nbody - 2) // 2
        assert all(staged), (name, staged)
        assert all(W0[c + "vstage"] == -1 for c in ("cf.", "cg.", "ch.", "cx."))
        for t in (0, 1, 2) + ((3,) if W["last_tier"] == 4 else ()):
            off, size = _regions(W, t)[0]["rowMisc"]
            assert 2 * size >= M.CAND_CAP, (name, t, size)


def test_half_turn_cases_tie_across_the_trips_of_a_large_hull():
    """What a non-strict `mx > bd` in hull_support_wave would change: an equal maximum in a LATER trip of 64 vertices replacing the first.  The half-turn cases of the
    130-vertex hull have such ties: along the centre line (the first support query) the largest projection is shared, to the last bit, by vertices of different trips."""
    from uhc_amd.model.mjcf import quat_to_mat
    m = M.family_model("ball130_house9")
    q, _, tags = M.family_cases("ball130_house9")
    V, _, _ = M.geom_hull(m, 1)
    across = 0
    for e in [k for k, t in enumerate(tags) if t == "quarter"][4:]:
        R = quat_to_mat(q[e, 3:7])
        assert set(np.unique(np.abs(R))) <= {0.0, 1.0}
        d = q[e, 7:10] - q[e, 0:3]
        l = R.T @ (d / np.linalg.norm(d))
        assert l[0] == 0
        proj = l[0] * V[:, 0] + l[1] * V[:, 1] + l[2] * V[:, 2]
        ties = np.nonzero(proj == proj.max())[0]
        print(f"MPR CASES ball130 half-turn case {e}: the largest projection is shared by vertices {ties.tolist()}")
        across += len(set(ties // 64)) > 1
    assert across >= 1


def test_drum_ties_lie_in_both_trips_and_the_first_wins():
    """The drum scene's claim, on the model as compiled: the bottom face's 40 vertices share one z to the last bit, the lowest-indexed of them is served by the first trip
    of 64 and others by the second -- where a non-strict comparison would let a later one replace it -- and the choice MATTERS: the oracle's qacc with another vertex order
    (the drum's vertex list reversed: the same hull) differs by far more than the bar the GPU file holds the device to."""
    import dataclasses
    from oracle.physics import OracleSim
    m, q, v = M.drum_scene()
    V, _, c = M.geom_hull(m, 1)
    assert len(V) == 2 * M.DRUM_SIDES and np.abs(c).max() < 1e-16
    low = np.nonzero(V[:, 2] == V[:, 2].min())[0]
    assert len(low) == M.DRUM_SIDES and low[0] < 64 and (low >= 64).any(), low
    ref = M.drum_reference()
    assert all(r["ncon"] == 1 and r["fail"] == 0 for r in ref)
    # the same hull with its bottom vertices listed in another order: rotate the drum's vertex block by one n-gon step about z (a symmetry of the hull)
    a = 2 * np.pi / M.DRUM_SIDES
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    mv = np.asarray(m.mesh_vert, dtype=np.float64).copy()
    mv[:len(V)] = V @ Rz.T
    m2 = dataclasses.replace(m, mesh_vert=mv)
    diff = []
    for e in range(len(q)):
        o = OracleSim(m2)
        o.set_state(q[e], v[e])
        diff.append(float(np.abs(o.get("qacc") - ref[e]["qacc"]).max()))
    print(f"MPR CASES drum: bottom vertices {low.tolist()}; |dqacc| of the oracle when another bottom vertex comes first: {['%.1e' % d for d in diff]}")
    assert max(diff) > 1e-3
