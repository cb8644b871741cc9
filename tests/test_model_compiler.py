"""Host model compiler (uhc_amd/model/mjcf.py): known-answer tests + the committed asset."""
import os

import numpy as np
import pytest

from tests.helpers import box_model, box_triangles, pendulum_model
from uhc_amd.model import mjcf

REF_XML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "humanoid_smpl_neutral_mesh", "humanoid_smpl_neutral_mesh.xml")


def test_box_mesh_mass_properties():
    tris = box_triangles(0.1, 0.2, 0.3, center=(1.0, -2.0, 0.5))
    v, f = mjcf.weld(tris)
    assert v.shape == (8, 3)
    vol, com, I = mjcf.polyhedron_mass_properties(v, f)
    assert vol == pytest.approx(8 * 0.1 * 0.2 * 0.3, rel=1e-12)
    np.testing.assert_allclose(com, [1.0, -2.0, 0.5], atol=1e-12)
    m = vol
    expect = m / 3 * np.diag([0.2 ** 2 + 0.3 ** 2, 0.1 ** 2 + 0.3 ** 2, 0.1 ** 2 + 0.2 ** 2])
    np.testing.assert_allclose(I, expect, atol=1e-12)


def test_tetrahedron_volume_and_com():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    vol, com, I = mjcf.polyhedron_mass_properties(v, f)
    assert vol == pytest.approx(1 / 6)
    np.testing.assert_allclose(com, [0.25, 0.25, 0.25], atol=1e-12)
    # Ixx of the unit right tetrahedron about its COM, unit density: 3/80 * vol * ... known value 1/80*... use integral check
    # integral (y^2+z^2) dV about origin = 2 * (1/60) ; shift to COM
    Ixx0 = 2.0 / 60.0
    assert I[0, 0] == pytest.approx(Ixx0 - vol * (0.25 ** 2 + 0.25 ** 2), rel=1e-12)


def test_pendulum_model_tables():
    m = pendulum_model()
    assert (m.nq, m.nv, m.nu, m.nbody, m.njnt) == (1, 1, 1, 2, 1)
    assert m.body_mass[1] == pytest.approx(1000 * 0.1 ** 3)
    np.testing.assert_allclose(m.body_ipos[1], [0, 0, -0.5], atol=1e-12)
    assert m.dof_parentid[0] == -1 and m.dof_madr.tolist() == [0, 1]
    # inertia about the hinge: I_com + m l^2 ; dof_invweight0 = 1/M
    I = m.body_mass[1] * (0.1 ** 2 + 0.1 ** 2) / 12 + m.body_mass[1] * 0.25
    assert m.dof_invweight0[0] == pytest.approx(1 / I, rel=1e-10)


def test_free_body_constants():
    m = box_model(0.1)
    assert (m.nq, m.nv, m.ngeom) == (7, 6, 2)
    mass = 1000 * 0.2 ** 3
    assert m.body_mass[1] == pytest.approx(mass)
    # free body: translational invweight = 1/m, rotational = 1/I
    I = mass * (0.2 ** 2 + 0.2 ** 2) / 12
    np.testing.assert_allclose(m.dof_invweight0, [1 / mass] * 3 + [1 / I] * 3, rtol=1e-9)
    np.testing.assert_allclose(m.body_invweight0[1], [1 / mass, 1 / I], rtol=1e-9)
    np.testing.assert_allclose(m.qpos0, [0, 0, 0.1, 1, 0, 0, 0])
    # hull graph: every box vertex has 3 axis neighbours + diagonals from the triangulation
    deg = np.diff(m.mesh_adjadr)
    assert deg.min() >= 3 and deg.sum() == m.nmeshadj


def test_asset_model_layout():
    from uhc_amd.sim import load_asset_model
    m = load_asset_model()
    assert (m.nq, m.nv, m.nu, m.nbody, m.njnt, m.ngeom, m.nM) == (76, 75, 69, 25, 70, 25, 1221)
    assert m.body_names[1] == "Pelvis" and m.body_names[-1] == "R_Hand"
    assert m.timestep == pytest.approx(0.00222222222)
    # longest dof chain Pelvis..Hand = 30
    depth = np.zeros(m.nv, dtype=int)
    for i in range(m.nv):
        depth[i] = 0 if m.dof_parentid[i] < 0 else depth[m.dof_parentid[i]] + 1
    assert depth.max() + 1 == 30
    # floor collides with every body geom, body geoms do not collide with each other
    assert m.geom_type[0] == mjcf.GEOM_PLANE and (m.geom_contype[1:] == 0).all() and (m.geom_conaffinity == 1).all()


def test_asset_matches_fresh_compile_of_reference_xml():
    """The committed asset against a fresh compile of the reference's humanoid MJCF (tests/golden/humanoid_smpl_neutral_mesh: the scene file and
    the 24 STL meshes it names, as the reference ships them)."""
    from uhc_amd.sim import load_asset_model
    a = load_asset_model()
    b = mjcf.compile_mjcf_file(REF_XML)
    for name in ("body_pos", "body_mass", "body_inertia", "body_ipos", "mesh_vert", "dof_invweight0", "body_invweight0", "jnt_range"):
        np.testing.assert_allclose(getattr(a, name), getattr(b, name), rtol=0, atol=1e-12, err_msg=name)
    assert a.body_names == b.body_names and a.actuator_names == b.actuator_names


def test_shape_to_model_generator_round_trip(model):
    """uhc_amd/smpllib/smpl_robot.py (the reference's Robot.load_from_skeleton pipeline): fed with the neutral asset's own hull vertices as
    'SMPL vertices' (one-hot skin weights, joints = body origins), the generator must give the asset back -- same tree and names, same bone
    offsets, the same masses up to the vertices the 50-vertex budget removes -- with body-body collisions and the two excludes switched on."""
    import numpy as np
    from uhc_amd.model.mjcf import kinematics_np, quat_to_mat
    from uhc_amd.smpllib.smpl_mujoco import SMPL_BONE_ORDER_NAMES
    from uhc_amd.smpllib.smpl_robot import Robot, SMPLBody, decimate_hull
    xpos, xquat, _, _ = kinematics_np(model, model.qpos0)
    verts, owner = [], []
    for g in range(model.ngeom):
        if model.geom_type[g] != 7:
            continue
        b = model.geom_bodyid[g]
        v = model.mesh_vert[model.geom_vertadr[g]:model.geom_vertadr[g] + model.geom_vertnum[g]] @ quat_to_mat(xquat[b]).T + xpos[b]
        verts.append(v)
        owner += [SMPL_BONE_ORDER_NAMES.index(model.body_names[b])] * len(v)
    verts = np.concatenate(verts)
    W = np.zeros((len(verts), 24))
    W[np.arange(len(verts)), owner] = 1
    joints = np.stack([xpos[model.body_names.index(n)] for n in SMPL_BONE_ORDER_NAMES])
    for ball in (False, True):
        r = Robot({"mesh": True, "ball": ball}, body_provider=lambda b, g: (verts, joints, W))
        r.load_from_skeleton(np.zeros(16), gender=[0])
        assert b"<mujoco" in r.export_xml_string()
        g = r.get_model()
        assert g.body_names == model.body_names and g.nbody == 25 and g.nv == 75 and g.nu == 69 and g.nq == (99 if ball else 76)
        np.testing.assert_allclose(g.body_pos, model.body_pos, atol=1e-4)  # the XML carries 4 decimals, like the reference's writer
        np.testing.assert_allclose(g.body_mass, model.body_mass, rtol=0.02)
        assert (g.geom_contype[1:] == 1).all() and g.nexclude == 2 and g.geom_vertnum.max() <= 50
        assert g.actuator_names == model.actuator_names
        if not ball:  # rel_joint_lm knee range (smpl_robot.py:1087-1092)
            j = g.joint_names.index("L_Knee_x")
            np.testing.assert_allclose(g.jnt_range[j], [-np.pi / 16, np.pi], atol=1e-4)
    # the vertex budget: a dense ellipsoid comes down to 50 hull vertices and keeps most of its volume
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(0)
    P = rng.normal(size=(800, 3))
    P = P / np.linalg.norm(P, axis=1)[:, None] * [0.1, 0.05, 0.2]
    D = decimate_hull(P, 50)
    assert len(D) == 50 and ConvexHull(D).volume > 0.85 * ConvexHull(P).volume
    # the SMPL forward pass itself needs the licensed model files
    import pytest
    with pytest.raises(FileNotFoundError):
        SMPLBody("/nonexistent")(np.zeros(10), 0)


def test_export_mjcf_round_trips_through_the_compiler(model):
    """export_mjcf (local coordinates, inline hull vertices; the form handed to a real MuJoCo in tests/test_mujoco_live.py) compiled
    again gives the same model: exactly with the inertial numbers written out, to the hull-vs-STL difference when mass properties are
    left to the reader (`density=`: the shipped STL hulls are convex only to ~1e-5 m)."""
    from uhc_amd.model.mjcf import ball_variant, compile_mjcf, export_mjcf, self_collision_variant
    for m in (self_collision_variant(model), ball_variant(model, damping=5.0)):
        r = compile_mjcf(export_mjcf(m))
        assert (r.nq, r.nv, r.nu, r.nbody, r.njnt, r.ngeom, r.nexclude) == (m.nq, m.nv, m.nu, m.nbody, m.njnt, m.ngeom, m.nexclude)
        for k in ("body_parentid", "dof_parentid", "dof_madr", "jnt_type", "geom_contype", "geom_conaffinity", "geom_condim", "actuator_dofid"):
            np.testing.assert_array_equal(getattr(r, k), getattr(m, k), err_msg=k)
        for k in ("body_pos", "body_quat", "body_mass", "body_inertia", "body_ipos", "jnt_pos", "jnt_axis", "jnt_range", "dof_armature", "dof_damping",
                  "dof_invweight0", "body_invweight0", "qpos0", "geom_margin", "geom_solref", "geom_solimp", "geom_friction"):
            np.testing.assert_allclose(getattr(r, k), getattr(m, k), atol=1e-12, err_msg=k)
        np.testing.assert_allclose(np.asarray(r.actuator_gear).reshape(m.nu, -1)[:, :1 if m.actuator_gear.ndim == 1 else 3],
                                   np.asarray(m.actuator_gear).reshape(m.nu, -1), atol=0)
        assert np.array_equal(np.sort(r.exclude_pair, axis=1), np.sort(m.exclude_pair, axis=1))
    d = compile_mjcf(export_mjcf(model, density=1000.0))
    np.testing.assert_allclose(d.body_mass, model.body_mass, rtol=2e-3)
    np.testing.assert_allclose(d.body_ipos, model.body_ipos, atol=1e-4)


def _recompile_scaled(model, s):
    """The per-body-scaled humanoid compiled FROM SCRATCH: hull of body b scaled by s_b about the body origin, bone offsets to its children
    by s_b, densities unchanged -- through the MJCF exporter and the compiler, i.e. mass properties re-integrated from the scaled meshes
    and the qpos0 constants recomputed, instead of the s^3 / s^5 shortcut of scale_model_per_body."""
    m = model.copy()
    par = np.asarray(model.body_parentid)
    m.body_pos = model.body_pos * np.where(par > 0, s[par], 1.0)[:, None]
    m.jnt_pos = model.jnt_pos * s[np.asarray(model.jnt_bodyid)][:, None]
    mv = model.mesh_vert.copy()
    for g in range(model.ngeom):
        if model.geom_type[g] == mjcf.GEOM_MESH:
            a, n = int(model.geom_vertadr[g]), int(model.geom_vertnum[g])
            mv[a:a + n] *= s[model.geom_bodyid[g]]
    m.mesh_vert = mv
    return mjcf.compile_mjcf(mjcf.export_mjcf(m, density=1000.0))


def test_scale_model_per_body_equals_a_recompile_of_the_scaled_meshes(model):
    """configs[3] (`bench.py --shapes`, smpl_shape): scale_model_per_body's closed-form scaling (mass ~ s^3, inertia ~ s^5, offsets ~ s,
    qpos0 constants recomputed) against a fresh compile of the scaled hulls.  The reference rebuilds the MuJoCo model from the new meshes
    for every shape (uhc/envs/humanoid_im.py:154-190); the two must agree up to the hull-vs-STL difference of the baseline itself."""
    from uhc_amd.model.mjcf import scale_model_per_body
    rng = np.random.default_rng(7)
    base = mjcf.compile_mjcf(mjcf.export_mjcf(model, density=1000.0))  # same route, unit scales: isolates the hull-vs-STL difference
    for _ in range(3):
        s = np.r_[1.0, rng.uniform(0.85, 1.15, size=model.nbody - 1)]
        a, b = scale_model_per_body(base, s), _recompile_scaled(model, s)
        np.testing.assert_allclose(a.body_pos, b.body_pos, atol=1e-12)
        np.testing.assert_allclose(a.body_mass, b.body_mass, rtol=1e-9)
        np.testing.assert_allclose(a.body_ipos, b.body_ipos, atol=1e-10)
        np.testing.assert_allclose(a.body_inertia, b.body_inertia, rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(a.geom_rbound, b.geom_rbound, rtol=1e-9)
        np.testing.assert_allclose(a.dof_invweight0, b.dof_invweight0, rtol=1e-7)
        np.testing.assert_allclose(a.body_invweight0, b.body_invweight0, rtol=1e-7)
        assert a.meaninertia == pytest.approx(b.meaninertia, rel=1e-9)
        # principal frames agree as rotations (quaternion sign and the order of near-equal moments aside): compare the inertia tensors
        for bd in range(1, model.nbody):
            Ra, Rb = mjcf.quat_to_mat(a.body_iquat[bd]), mjcf.quat_to_mat(b.body_iquat[bd])
            np.testing.assert_allclose(Ra @ np.diag(a.body_inertia[bd]) @ Ra.T, Rb @ np.diag(b.body_inertia[bd]) @ Rb.T, atol=1e-9)
        # hull vertices: same sets (the recompile reorders them through qhull)
        for g in range(model.ngeom):
            if model.geom_type[g] == mjcf.GEOM_MESH:
                va = a.mesh_vert[a.geom_vertadr[g]:a.geom_vertadr[g] + a.geom_vertnum[g]]
                vb = b.mesh_vert[b.geom_vertadr[g]:b.geom_vertadr[g] + b.geom_vertnum[g]]
                assert len(va) == len(vb)
                np.testing.assert_allclose(va[np.lexsort(va.T)], vb[np.lexsort(vb.T)], atol=1e-12)
    # and the mass-weighted identities the docstring promises, on the shipped asset itself
    s = np.r_[1.0, rng.uniform(0.85, 1.15, size=model.nbody - 1)]
    o = scale_model_per_body(model, s)
    np.testing.assert_allclose(o.body_mass, model.body_mass * s ** 3, rtol=1e-14)
    np.testing.assert_allclose(o.body_inertia, model.body_inertia * (s ** 5)[:, None], rtol=1e-14)
    assert o.nq == model.nq and np.array_equal(o.dof_madr, model.dof_madr)


def test_pose_body_and_height_fix():
    """fix_height_smpl_vanilla (uhc/data_process/process_amass_db.py:194-219) through a body provider: linear blend skinning on the SMPL
    tree (known answers: a knee bent by 90 degrees carries its own vertices about the knee joint, a root yaw turns the body about the
    pelvis), then the lowest vertex of frame 0 at z = 0 -- hooked into process_qpos_list (`fix_height=`)."""
    from uhc_amd.data_loaders.synthetic import make_synthetic_body_provider
    from uhc_amd.data_process.process_amass_db import process_qpos_list
    from uhc_amd.smpllib.smpl_robot import make_fix_height, pose_body
    J = np.array([[0.1 * j, 0.0, 1.0 - 0.03 * j] for j in range(24)])
    v = np.array([J[4] + [0, 0, -0.2], J[0] + [0, 0.1, 0]])
    W = np.zeros((2, 24))
    W[0, 4] = W[1, 0] = 1
    pose = np.zeros((24, 3))
    pose[4] = [np.pi / 2, 0, 0]
    np.testing.assert_allclose(pose_body(v, J, W, pose) - v, [[0, 0.2, 0.2], [0, 0, 0]], atol=1e-15)
    pose = np.zeros((24, 3))
    pose[0] = [0, 0, np.pi / 2]
    np.testing.assert_allclose(pose_body(v, J, W, pose)[1] - J[0], [-0.1, 0, 0], atol=1e-15)
    # blended weights: a vertex half on a rotating joint, half on its parent moves half way
    W2 = np.zeros((1, 24))
    W2[0, 4] = W2[0, 1] = 0.5
    pose = np.zeros((24, 3))
    pose[4] = [np.pi / 2, 0, 0]
    np.testing.assert_allclose(pose_body(v[:1], J, W2, pose) - v[:1], [[0, 0.1, 0.1]], atol=1e-15)
    # the hook: every kept clip starts with its lowest vertex on the floor
    prov = make_synthetic_body_provider()
    rng = np.random.default_rng(0)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "uhc_amd", "assets", "standing_neutral.npz"))
    poses = np.tile(z["pose_aa"][10], (40, 1)) + rng.normal(scale=0.02, size=(40, 72))
    db = [("ACCAD_s1_walk", {"poses": poses, "trans": np.tile([0.3, -0.2, 1.7], (40, 1)), "betas": rng.normal(size=16), "gender": "female", "mocap_framerate": 60.0})]
    res = process_qpos_list(db, {}, fix_height=make_fix_height(prov), log=lambda *a: None)
    (k, c), = res.items()
    assert c["height_fixed"] is True and c["pose_aa"].shape[0] == 20
    verts, joints, Wt = prov(c["beta"][:10], 2)
    low = (pose_body(verts, joints, Wt, c["pose_aa"][0]) + c["trans"][0])[:, 2].min()
    assert abs(low) < 1e-12 and np.ptp(c["trans"][:, 2]) == 0 and c["trans"][0, 0] == 0.3
