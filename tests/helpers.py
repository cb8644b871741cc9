"""Shared builders for tests (synthetic MJCF models written for this repo)."""
import numpy as np

from uhc_amd.model.shapes import box_triangles, hull_triangles, prism_triangles  # noqa: F401  (re-exported for the tests)


PENDULUM_XML = """
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="0.0005"/>
  <default><geom contype="0" conaffinity="0" margin="0.001"/></default>
  <asset><mesh name="bob" file="unused.stl"/></asset>
  <worldbody>
    <body name="arm" pos="0 0 2">
      <joint name="hinge" type="hinge" axis="0 1 0" pos="0 0 0"/>
      <geom type="mesh" mesh="bob"/>
    </body>
  </worldbody>
  <actuator><motor name="m" joint="hinge" gear="1"/></actuator>
</mujoco>
"""

BOX_ON_PLANE_XML = """
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom contype="1" conaffinity="1" condim="3" margin="0.001"/></default>
  <asset><mesh name="box" file="unused.stl"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="10 10 0.1" pos="0 0 0"/>
    <body name="box" pos="0 0 0.1">
      <joint name="root" type="free"/>
      <geom type="mesh" mesh="box" condim="1"/>
    </body>
  </worldbody>
</mujoco>
"""


def pendulum_model(length=0.5, half=0.05):
    from uhc_amd.model.mjcf import compile_mjcf
    tris = box_triangles(half, half, half, center=(0, 0, -length))
    return compile_mjcf(PENDULUM_XML, meshes={"bob": tris})


def box_model(half=0.1):
    from uhc_amd.model.mjcf import compile_mjcf
    return compile_mjcf(BOX_ON_PLANE_XML, meshes={"box": box_triangles(half, half, half)})


def weld_statue(model, qpos, *, friction=None, extra_geom_attr=""):
    """The articulated humanoid frozen in the pose `qpos` as ONE free rigid body carrying all of its hulls (a statue): what is left
    of the model when every hinge is welded.  Used by the behavioural contact tests: a statue whose centre of mass projects well
    inside its support polygon has to keep standing, whatever the controller would do."""
    from uhc_amd.model.mjcf import compile_mjcf, kinematics_np, quat_to_mat
    xpos, xquat, _, _ = kinematics_np(model, np.asarray(qpos, dtype=np.float64))
    Rr, pr = quat_to_mat(xquat[1]), xpos[1]
    meshes, geoms = {}, []
    for g in range(model.ngeom):
        if model.geom_type[g] != 7:
            continue
        b = model.geom_bodyid[g]
        v = model.mesh_vert[model.geom_vertadr[g]:model.geom_vertadr[g] + model.geom_vertnum[g]]
        w = v @ quat_to_mat(xquat[b]).T + xpos[b]          # world
        meshes[f"h{g}"] = hull_triangles((w - pr) @ Rr)      # root-body frame
        geoms.append(f'<geom type="mesh" mesh="h{g}" {extra_geom_attr}/>')
    fr = "" if friction is None else f'friction="{friction} 0.005 0.0001"'
    xml = f"""
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="{model.timestep}"/>
  <default><geom contype="0" conaffinity="1" condim="1" margin="0.001"/></default>
  <asset>{''.join(f'<mesh name="{k}" file="unused.stl"/>' for k in meshes)}</asset>
  <worldbody>
    <geom name="floor" type="plane" size="10 10 0.1" pos="0 0 0" contype="1" conaffinity="1" condim="3" {fr}/>
    <body name="statue" pos="{pr[0]} {pr[1]} {pr[2]}" quat="{xquat[1][0]} {xquat[1][1]} {xquat[1][2]} {xquat[1][3]}">
      <joint name="root" type="free"/>
      {''.join(geoms)}
    </body>
  </worldbody>
</mujoco>
"""
    return compile_mjcf(xml, meshes=meshes)


def passive_ctrl(model, n_substeps=1):
    """Controller description of an unactuated / torque-driven model for SimBatch: action = raw torques (none when nu == 0)."""
    from uhc_amd._capi import ctrl_desc
    nu = max(int(model.nu), 1)
    return ctrl_desc(n_substeps=n_substeps, action_type=1, meta_pd=0, rfc_mode=0, action_dim=nu, jkp=np.zeros(nu), jkd=np.zeros(nu),
                     torque_lim=np.full(nu, 1e9), a_scale=np.full(nu, 0.01))


TWO_BOX_XML = """
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom contype="1" conaffinity="1" condim="1" margin="0.001"/></default>
  <asset><mesh name="a" file="unused.stl"/><mesh name="b" file="unused.stl"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="10 10 0.1" pos="0 0 0" condim="3"/>
    <body name="A" pos="0 0 0.1">
      <joint name="ra" type="free"/>
      <geom type="mesh" mesh="a"/>
    </body>
    <body name="B" pos="0 0 0.3">
      <joint name="rb" type="free"/>
      <geom type="mesh" mesh="b"/>
    </body>
  </worldbody>
</mujoco>
"""


def two_box_model(ha=0.1, hb=0.06):
    """Two free boxes (meshes) above the plane: box-box contacts go through the convex-convex (MPR) narrow phase, two kinematic trees."""
    from uhc_amd.model.mjcf import compile_mjcf
    return compile_mjcf(TWO_BOX_XML, meshes={"a": box_triangles(ha, ha, ha), "b": box_triangles(hb, hb, hb)})


def caterpillar_model(n_seg=27, half=0.1, gap=0.02):
    """A serial chain lying on the floor: a free root box and n_seg - 1 boxes behind it, each on ONE hinge about y -- the dof chain of the last box has 6 + (n_seg - 1) entries
    (32 with 27 segments: the deepest chain uhc_batch_create accepts).  Every box meets the floor with its four bottom vertices at slightly different heights (no exact ties for the
    plane-mesh narrow phase), the boxes do not collide with each other (contype 0): 16 pyramid rows per resting box, 432 for the whole animal."""
    from uhc_amd.model.mjcf import compile_mjcf
    tris = box_triangles(half, half, half)
    v = tris.reshape(-1, 3).copy()
    dz = {(-1, -1): 0.0, (1, -1): -0.0003, (1, 1): -0.0006, (-1, 1): 0.0003}
    for k in range(v.shape[0]):
        if v[k, 2] < 0:
            v[k, 2] += dz[(int(np.sign(v[k, 0])), int(np.sign(v[k, 1])))]
    tris = v.reshape(-1, 3, 3)
    step = 2 * half + gap
    body = ""
    for k in range(n_seg - 1, 0, -1):
        body = f'<body name="s{k}" pos="{step} 0 0"><joint name="j{k}" type="hinge" axis="0 1 0" pos="{-step / 2} 0 0"/><geom type="mesh" mesh="seg"/>{body}</body>'
    xml = f"""
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom contype="0" conaffinity="1" condim="3" margin="0.001"/></default>
  <asset><mesh name="seg" file="unused.stl"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="20 20 0.1" pos="0 0 0" contype="1" conaffinity="1"/>
    <body name="s0" pos="0 0 {half}">
      <joint name="root" type="free"/>
      <geom type="mesh" mesh="seg"/>
      {body}
    </body>
  </worldbody>
</mujoco>
"""
    return compile_mjcf(xml, meshes={"seg": tris})


def slider_model(axis=(1.0, 0.3, 0.2), limit=(-0.3, 0.4)):
    """Slide joints on every side of a hinge, no contacts (contype 0): a 1 kg cart on a LIMITED slide whose axis is no coordinate axis (an unrotated or transposed axis
    shows) and whose body carries a non-identity quat; the cart carries a pendulum arm on a hinge, and the arm a bob on a second slide -- a slide below a rotating parent, and
    slide, hinge and slide dofs in one dof chain (the L^-T back substitution crosses both motion subspaces).  One motor per joint."""
    from uhc_amd.model.mjcf import compile_mjcf
    tris = box_triangles(0.03, 0.03, 0.03)
    xml = f"""
<mujoco>
  <compiler angle="radian" coordinate="local"/>
  <option timestep="0.002"/>
  <default><geom contype="0" conaffinity="0" margin="0.001"/></default>
  <asset><mesh name="cube" file="unused.stl"/></asset>
  <worldbody>
    <body name="cart" pos="0.1 -0.2 1.5" quat="0.9 0.1 0.3 0.2">
      <inertial pos="0.01 0.02 -0.01" mass="1" diaginertia="0.02 0.015 0.01"/>
      <joint name="rail" type="slide" axis="{axis[0]} {axis[1]} {axis[2]}" pos="0 0 0" limited="true" range="{limit[0]} {limit[1]}"/>
      <geom type="mesh" mesh="cube"/>
      <body name="arm" pos="0.02 0.05 -0.1" quat="0.98 0.05 -0.1 0.15">
        <inertial pos="0.01 0 -0.25" mass="0.5" diaginertia="0.012 0.011 0.002"/>
        <joint name="pivot" type="hinge" axis="0.1 1 0.2" pos="0 0 0.03"/>
        <geom type="mesh" mesh="cube"/>
        <body name="bob" pos="0 0.01 -0.3" quat="0.95 -0.2 0.1 0.1">
          <inertial pos="0 0.01 0.02" mass="0.3" diaginertia="0.003 0.002 0.002"/>
          <joint name="telescope" type="slide" axis="0.2 -0.1 1" pos="0.01 0 0"/>
          <geom type="mesh" mesh="cube"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator><motor name="m_rail" joint="rail" gear="1"/><motor name="m_pivot" joint="pivot" gear="1"/><motor name="m_telescope" joint="telescope" gear="1"/></actuator>
</mujoco>
"""
    return compile_mjcf(xml, meshes={"cube": tris})


def cart_model(axis=(0.0, 0.0, 1.0), limit=None):
    """One 1 kg body on ONE slide joint along `axis`, timestep 0.002, no contacts: the scene of the closed forms (weight against friction loss, a spring's period, a limit)."""
    from uhc_amd.model.mjcf import compile_mjcf
    lim = "" if limit is None else f'limited="true" range="{limit[0]} {limit[1]}"'
    xml = f"""
<mujoco>
  <compiler angle="radian" coordinate="local"/>
  <option timestep="0.002"/>
  <default><geom contype="0" conaffinity="0" margin="0.001"/></default>
  <asset><mesh name="cube" file="unused.stl"/></asset>
  <worldbody>
    <body name="cart" pos="0.3 0.2 1">
      <inertial pos="0 0 0" mass="1" diaginertia="0.01 0.01 0.01"/>
      <joint name="rail" type="slide" axis="{axis[0]} {axis[1]} {axis[2]}" pos="0 0 0" {lim}/>
      <geom type="mesh" mesh="cube"/>
    </body>
  </worldbody>
  <actuator><motor name="m_rail" joint="rail" gear="1"/></actuator>
</mujoco>
"""
    return compile_mjcf(xml, meshes={"cube": box_triangles(0.03, 0.03, 0.03)})


def with_passives(model, frictionloss=None, stiffness=None, qpos_spring=None):
    """`model` with other passive joint terms (a dataclasses.replace: nothing derived depends on them).  Each of `frictionloss`, `stiffness` and `qpos_spring` is a scalar
    -- given to every hinge and slide joint, the joints whose springs and friction loss the models of the configs set -- or an array with one value per joint, or one per dof
    (`qpos_spring`: per entry of qpos).  None leaves the model's own values."""
    import dataclasses
    jt, ja, da = np.asarray(model.jnt_type), np.asarray(model.jnt_qposadr), np.asarray(model.jnt_dofadr)
    scalar_jnt = (jt == 2) | (jt == 3)  # slide, hinge
    dofs_of = [np.flatnonzero(np.asarray(model.dof_jntid) == j) for j in range(model.njnt)]
    new = {}
    if frictionloss is not None:
        f = np.asarray(frictionloss, dtype=np.float64)
        out = np.asarray(model.dof_frictionloss, dtype=np.float64).copy()
        if f.ndim == 0:
            for j in np.flatnonzero(scalar_jnt):
                out[dofs_of[j]] = f
        elif f.shape == (model.nv,):
            out = f.copy()
        else:
            assert f.shape == (model.njnt,), f.shape
            for j in range(model.njnt):
                out[dofs_of[j]] = f[j]
        new["dof_frictionloss"] = out
    if stiffness is not None:
        k = np.asarray(stiffness, dtype=np.float64)
        out = np.asarray(model.jnt_stiffness, dtype=np.float64).copy()
        if k.ndim == 0:
            out[scalar_jnt] = k
        elif k.shape == (model.njnt,):
            out = k.copy()
        else:  # per dof: a joint takes the value of its first dof
            assert k.shape == (model.nv,), k.shape
            out = k[da].copy()
        new["jnt_stiffness"] = out
    if qpos_spring is not None:
        r = np.asarray(qpos_spring, dtype=np.float64)
        out = np.asarray(model.qpos_spring, dtype=np.float64).copy()
        if r.ndim == 0:
            out[ja[scalar_jnt]] = r
        elif r.shape == (model.nq,) and model.nq != model.njnt:
            out = r.copy()
        else:
            assert r.shape == (model.njnt,), r.shape
            out[ja[scalar_jnt]] = r[scalar_jnt]
        new["qpos_spring"] = out
    return dataclasses.replace(model, **new)
