"""Case tables for the env kernels' branch edges (tests/test_gpu_env_edges.py) and the float64 oracle evaluated on a given state.
No GPU in here: the builders are numpy (torch on the CPU only for Humanoid.qpos_fk), tests/test_env_edge_cases_cpu.py checks on
stand-in states that every named case reaches the branch it claims.

A `state` is what the device holds after a reset or a step -- dict(qpos, qvel, xpos (nbody, 3), xquat (nbody, 4), xipos (nbody, 3)) --
and a `window` is the (len, FRAME_STRIDE) slice of the clip bank an env tracks.  Every oracle call takes the two and nothing else."""
import math

import numpy as np

from oracle import env_oracle as E
from uhc_amd.sim import FR, FRAME_STRIDE, pack_expert_frames
from uhc_amd.utils.transformation import quaternion_multiply

PI = math.pi
BASE_UNIT = np.array([math.sqrt(0.5), math.sqrt(0.5), 0.0, 0.0])  # the base rotation the SMPL root carries (x by 90 degrees)
POISON = 1.0e3   # value of the frames no window owns: an index off by one reads it
N_CLIPS = 5
CLIP_PAD = [37, 5, 113, 19, 61]  # unowned frames in front of every clip: large, different clip_start offsets
FUT_FRAMES, FUT_SKIP = 3, 4      # observation v3
OBS_KINDS = [0, 1, 2, 3, 4, 5, 6, "ball"]
OBS_DIM = {0: 220, 1: 784, 2: 657, 3: 3 * 657, 4: 643, 5: 653, 6: 401, "ball": 534}
K_NUDGE, BAR_FACTOR, BAR_FLOOR = 8, 16.0, 1e-14


def axis_quat(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.r_[math.cos(0.5 * angle), math.sin(0.5 * angle) * a]


def root_quat(yaw, pitch=0.0, roll=0.0, sign=1.0, scale=1.0):
    """Root quaternion whose base-rotation-free part is Rz(yaw) Ry(pitch) Rx(roll); `sign` picks q or -q, `scale` its norm."""
    q = quaternion_multiply(quaternion_multiply(axis_quat(yaw, [0, 0, 1]), axis_quat(pitch, [0, 1, 0])), axis_quat(roll, [1, 0, 0]))
    return sign * scale * quaternion_multiply(q, BASE_UNIT)


def clip_beta_rows():
    r = np.random.default_rng(5)
    return np.concatenate([r.normal(size=(N_CLIPS, 16)), np.array([[2.0], [1.0], [0.0], [2.0], [1.0]])], axis=1)


# --------------------------------------------------------------------------------------------------------------- observation table
def obs_cases():
    """One dict per env: rows (len, 76) of qpos -- row 0 the state, row 1 the target, further rows the look-ahead frames --, the
    state's qvel (75), `claims` (what tests/test_env_edge_cases_cpu.py asserts the oracle reaches) and optional record overrides."""
    rng = np.random.default_rng(20)
    cases = []

    def pose(rootq, z=0.92, joints=None, xy=None):
        q = np.zeros(76)
        q[:2] = rng.normal(scale=0.7, size=2) if xy is None else xy
        q[2] = z
        q[3:7] = rootq
        q[7:] = rng.normal(scale=0.35, size=69) if joints is None else joints
        return q

    def add(name, rows, claims=(), qvel=None, override=None):
        cases.append(dict(name=name, rows=np.asarray(rows), qvel=rng.normal(scale=1.5, size=75) if qvel is None else qvel, claims=tuple(claims),
                          override=override))

    # root yaw through the four quadrants, next to 0 and to +-pi, each as q and -q (w < 0; z < 0 before heading()'s swap)
    for yaw in (1e-3, -1e-3, 0.7, -0.7, 2.2, -2.2, PI - 1e-3, -(PI - 1e-3)):
        for sign in (1.0, -1.0):
            claims = ["z_neg"] if (yaw < 0) == (sign > 0) else []
            claims += ["w_neg"] if sign < 0 else []
            add(f"yaw{yaw:+.4f}{'q' if sign > 0 else '-q'}", [pose(root_quat(yaw, sign=sign)), pose(root_quat(yaw + 0.4, 0.1, -0.05, sign=-sign), z=0.88)], claims)
    # heading differences beyond +-pi: with the acos heading of v0-v4 (range [0, 2 pi]) and with the atan2 heading of v5 / v6
    add("wrap_acos_hi", [pose(root_quat(0.3)), pose(root_quat(-0.8))], ["acos_raw_above_pi"])
    add("wrap_acos_lo", [pose(root_quat(-0.8)), pose(root_quat(0.3))], ["acos_raw_below_minus_pi"])
    add("wrap_atan_hi", [pose(root_quat(-2.5)), pose(root_quat(2.5))], ["atan_raw_above_pi"])
    add("wrap_atan_lo", [pose(root_quat(2.5)), pose(root_quat(-2.5))], ["atan_raw_below_minus_pi"])
    # large pitch / roll; the last two bring sqrt(w^2 + z^2) down to 1.7e-3: of the base-rotation-free quaternion (v1-v4, ball), of the raw one (v0)
    d = PI / 180
    add("pitch89", [pose(root_quat(0.5, 89 * d, 0.0)), pose(root_quat(0.9, -70 * d, 0.2))])
    add("roll89", [pose(root_quat(-1.1, 0.0, 89 * d)), pose(root_quat(-0.6, 0.3, -80 * d))])
    add("pitch60_roll-75", [pose(root_quat(2.0, 60 * d, -75 * d)), pose(root_quat(2.4, 85 * d, 40 * d))])
    add("small_hq_crq", [pose(root_quat(0.7, 0.0, 179.8 * d)), pose(root_quat(1.0, 0.0, 150 * d))], ["hq_small_crq"])
    add("small_hq_rootq", [pose(root_quat(0.7, 0.0, 89.8 * d)), pose(root_quat(0.4, 0.2, 60 * d))], ["hq_small_rootq"])
    # root rotated by pi about an axis: the root body's world quaternion has w == 0.0 exactly, the observation takes the target's quaternions
    # (the target's world quaternions, which then stand in for the current ones, are scaled off the unit sphere: conj / |q| and conj / |q|^2 differ on them)
    def off_unit_wbquat(fr):
        o, n = FR["wbquat"]
        fr[1, o:o + n] = (fr[1, o:o + n].reshape(-1, 4) * (1.0 + 1e-3 * np.where(np.arange(n // 4) % 2 == 0, 1.0, -1.0))[:, None]).ravel()

    add("unset_q", [pose(np.array([0.0, 0.6, 0.0, 0.8])), pose(root_quat(1.3, 0.2, 0.1))], ["unset"], override=off_unit_wbquat)
    add("unset_-q", [pose(-np.array([0.0, 0.6, 0.0, 0.8])), pose(root_quat(-0.3, -0.2, 0.4))], ["unset"], override=off_unit_wbquat)
    # root quaternion off the unit sphere
    add("norm_1.001", [pose(root_quat(0.8, 0.3, -0.2, scale=1.001)), pose(root_quat(1.1, 0.1, 0.1, scale=0.999))])
    add("norm_0.999", [pose(root_quat(-1.9, -0.4, 0.3, scale=0.999)), pose(root_quat(-2.3, 0.2, 0.0, scale=1.001))])
    # joint angles on and beyond the range limits of the asset (+-pi, +-4 pi for some), +-pi itself, joint velocities +-50
    from uhc_amd.sim import load_asset_model
    rng_j = np.asarray(load_asset_model().jnt_range, dtype=np.float64)[1:]
    lo, hi = rng_j[:, 0], rng_j[:, 1]
    alt = np.where(np.arange(69) % 2 == 0, 1.0, -1.0)
    v50 = np.r_[rng.normal(size=6), 50.0 * alt]
    add("joints_hi", [pose(root_quat(0.2), joints=hi), pose(root_quat(0.3), joints=lo)], qvel=v50)
    add("joints_lo", [pose(root_quat(-0.2), joints=lo), pose(root_quat(0.1), joints=np.where(alt > 0, hi, lo))], qvel=-v50)
    add("joints_alt_pi", [pose(root_quat(1.2), joints=PI * alt), pose(root_quat(1.0), joints=-PI * alt)], qvel=np.r_[-v50[:6], 50.0 * alt[::-1] * np.where(np.arange(69) % 3 == 0, -1.0, 1.0)])
    add("joints_beyond", [pose(root_quat(-2.9), joints=np.where(alt > 0, hi + 0.5, lo - 0.5)), pose(root_quat(3.0), joints=np.where(alt > 0, lo - 0.9, hi + 0.9))],
        qvel=np.r_[v50[:6], -50.0 * alt])
    # window geometry: len 1 (target = state), 2, 3; for v3 (look-aheads 1, 5, 9): all clamped, only the last clamped, none clamped
    add("len1", [pose(root_quat(0.6, 0.1, 0.1))], ["len1", "v3_all_clamped"])
    add("len2", [pose(root_quat(-0.4)), pose(root_quat(-0.9, 0.2))], ["v3_all_clamped"])
    add("len3", [pose(root_quat(1.7))] + [pose(root_quat(1.7 + 0.3 * k, 0.1 * k)) for k in (1, 2)])
    add("len7", [pose(root_quat(-1.4))] + [pose(root_quat(-1.4 + 0.2 * k, 0.05 * k)) for k in range(1, 7)], ["v3_last_clamped"])
    add("len12", [pose(root_quat(2.8))] + [pose(root_quat(2.8 + 0.2 * k, -0.05 * k)) for k in range(1, 12)], ["v3_none_clamped"])
    return cases


def frames_of_rows(humanoid, rows):
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.shape[0] == 1:  # (qpos_fk has no velocities for a single frame: a clip of one frame gets zero qvel / bangvel)
        fr = pack_expert_frames(humanoid.qpos_fk(torch.from_numpy(np.repeat(rows, 2, axis=0))))[:1]
        for k in ("qvel", "bangvel"):
            fr[:, FR[k][0]:FR[k][0] + FR[k][1]] = 0.0
        return fr
    return pack_expert_frames(humanoid.qpos_fk(torch.from_numpy(rows)))


def obs_windows(humanoid, cases):
    """The cases' frame records: Humanoid.qpos_fk on the crafted rows, the state's qvel in the slot a reset reads it from."""
    wins = []
    q0, qn = FR["qvel"]
    for c in cases:
        fr = frames_of_rows(humanoid, c["rows"])
        fr[min(1, fr.shape[0] - 1), q0:q0 + qn] = c["qvel"]
        if c["override"] is not None:
            c["override"](fr)
        wins.append(fr)
    return wins


def assemble_bank(windows):
    """Windows dealt round-robin onto N_CLIPS clips, unowned POISON frames in front of every clip and at the very end.
    Returns frames, clip_start, per window (clip id, first frame inside the clip, len)."""
    per_clip = [[np.full((CLIP_PAD[c], FRAME_STRIDE), POISON)] for c in range(N_CLIPS)]
    fill = list(CLIP_PAD)
    where = []
    for i, w in enumerate(windows):
        c = i % N_CLIPS
        where.append((c, fill[c], w.shape[0]))
        per_clip[c].append(w)
        fill[c] += w.shape[0]
    clip_start = np.r_[0, np.cumsum(fill)[:-1]].astype(np.int32)
    frames = np.concatenate([np.concatenate(p) for p in per_clip] + [np.full((1, FRAME_STRIDE), POISON)])
    return frames, clip_start, np.array(where, dtype=np.int32)


def env_ids_for(n_cases, n_env, seed=3):
    """A permuted strict subset of the env ids, one per case."""
    assert n_cases < n_env
    return np.random.default_rng(seed).permutation(n_env)[:n_cases].astype(np.int32)


# --------------------------------------------------------------------------------------------------------------- window / state <-> oracle
def expert_of_window(win):
    ex = {k: win[:, o:o + n] for k, (o, n) in FR.items()}
    ex["len"] = win.shape[0]
    b0 = FR["bquat"][0]
    ex["qpos_quat"] = np.concatenate([win[:, :7], win[:, b0 + 4:b0 + 96]], axis=1)  # the ball-joint expert pose (uhc_env.hip: expert_qpos)
    return ex


def stand_in_state(win, ball=False, frame=0):
    """The state a reset onto `win` would produce if the device's kinematics equalled qpos_fk: the CPU tests' "device"."""
    ex = expert_of_window(win)
    L = win.shape[0]
    return dict(qpos=(ex["qpos_quat"] if ball else ex["qpos"])[frame].copy(), qvel=ex["qvel"][min(frame + 1, L - 1)].copy(),
                xpos=np.concatenate([np.zeros((1, 3)), ex["wbpos"][frame].reshape(-1, 3)]),
                xquat=np.concatenate([[[1.0, 0, 0, 0]], ex["wbquat"][frame].reshape(-1, 4)]),
                xipos=np.concatenate([np.zeros((1, 3)), ex["body_com"][frame].reshape(-1, 3)]))


STATE_KEYS = ("qpos", "qvel", "xpos", "xquat", "xipos")


def oracle_obs(kind, st, win, cur_t, beta17):
    ex = expert_of_window(win)
    beta, gender = beta17[:16], beta17[16]
    q, v, xp, xq, xi = (st[k] for k in STATE_KEYS)
    if kind == "ball":
        return E.full_obs_v2_quat(q, v, xp, xq, ex, cur_t, 0, beta, gender)
    if kind == 0:
        return E.full_obs_v0(q, v, ex, cur_t, 0, obs_heading=True, root_deheading=True, obs_phase=True)
    if kind == 1:
        return E.full_obs_v1(q, v, xp, xq, xi, ex, cur_t, 0)
    if kind == 2:
        return E.full_obs_v2(q, v, xp, xq, ex, cur_t, 0, beta, gender)
    if kind == 3:
        return E.full_obs_v3(q, v, xp, xq, ex, cur_t, 0, beta, gender, fut_frames=FUT_FRAMES, skip=FUT_SKIP)
    if kind == 4:
        return E.full_obs_v4(q, v, xp, xq, ex, cur_t, 0, beta, gender)[0]
    if kind == 5:
        return E.full_obs_v5(q, v, xp, xq, ex, cur_t, 0, beta, gender)
    if kind == 6:
        return E.full_obs_v6(q, v, xp, ex, cur_t, 0, beta, gender)
    raise AssertionError(kind)


def obs_branches(st, win, cur_t=0):
    """Which side of every switch of the observation code this (state, window) is on."""
    L = win.shape[0]
    rootq = st["qpos"][3:7]
    crq = E.remove_base_rot(rootq)
    trq = E.remove_base_rot(win[E.expert_index(cur_t + 1, 0, L), 3:7])

    def acos_heading(q):  # get_heading before the wrap, with the sign of z it starts from
        return 2 * math.acos((q[0] if q[3] >= 0 else -q[0]) / math.hypot(q[0], q[3]))

    raw_a = acos_heading(trq) - acos_heading(crq)
    raw_n = E.get_heading_new(trq) - E.get_heading_new(crq)
    idx = [cur_t + 1 + k * FUT_SKIP for k in range(FUT_FRAMES)]
    return dict(z_neg=bool(crq[3] < 0), z_neg_root=bool(rootq[3] < 0), z_neg_target=bool(trq[3] < 0), w_neg=bool(crq[0] < 0),
                acos_raw=raw_a, acos_wrap=int(raw_a > PI) - int(raw_a < -PI), atan_raw=raw_n, atan_wrap=int(raw_n > PI) - int(raw_n < -PI),
                hq_crq=math.hypot(crq[0], crq[3]), hq_rootq=math.hypot(rootq[0], rootq[3]), hq_trq=math.hypot(trq[0], trq[3]),
                unset=bool(st["xquat"][1, 0] == 0), clamped=tuple(i > L - 1 for i in idx), target_is_state=L == 1)


def obs_sides(st, win, cur_t=0):
    b = obs_branches(st, win, cur_t)
    return (b["z_neg"], b["z_neg_root"], b["z_neg_target"], b["acos_wrap"], b["atan_wrap"], b["unset"])


# --------------------------------------------------------------------------------------------------------------- tolerance from the oracle itself
def nudge(a, rng):
    """Every entry one float64 step up or down, at random.  Exact zeros stay: a rounding error is relative, and the `unset` switch tests for one."""
    a = np.asarray(a, dtype=np.float64)
    up = rng.integers(0, 2, size=a.shape).astype(bool)
    return np.where(a == 0.0, a, np.nextafter(a, np.where(up, np.inf, -np.inf)))


def measured_bar(fn, arrays, seed, side=None):
    """fn(*arrays) -> vector.  Returns (reference value, per-entry bar, excluded): the bar is BAR_FACTOR x the spread of the oracle over the
    inputs and K_NUDGE copies of them moved by one float64 step, plus BAR_FLOOR x max(1, |value|); `excluded` says a copy changed `side`."""
    rng = np.random.default_rng(seed)
    ref = np.asarray(fn(*arrays), dtype=np.float64)
    outs, sides = [ref], [side(*arrays) if side else None]
    for _ in range(K_NUDGE):
        moved = [nudge(a, rng) for a in arrays]
        outs.append(np.asarray(fn(*moved), dtype=np.float64))
        sides.append(side(*moved) if side else None)
    outs = np.stack(outs)
    bar = BAR_FACTOR * (outs.max(0) - outs.min(0)) + BAR_FLOOR * np.maximum(1.0, np.abs(ref))
    return ref, bar, any(s != sides[0] for s in sides)


def obs_reference(kind, st, win, cur_t, beta17, seed):
    def unpack(q, v, xp, xq, xi, w):
        return dict(qpos=q, qvel=v, xpos=xp, xquat=xq, xipos=xi), w

    arrays = [st[k] for k in STATE_KEYS] + [win]
    return measured_bar(lambda *a: oracle_obs(kind, *unpack(*a), cur_t, beta17), arrays, seed, side=lambda *a: obs_sides(*unpack(*a), cur_t))


# --------------------------------------------------------------------------------------------------------------- reward table
REWARD_W = dict(w_p=0.3, w_v=0.1, w_e=0.45, w_c=0.1, w_vf=0.05, k_p=0.01, k_v=0.005, k_e=5.0, k_c=100.0, k_vf=1.0)
REWARD_W23 = dict(k_p=0.1, k_wp=0.1, k_v=0.004, k_j=60.0, k_c=80.0, k_vf=0.7, w_p=0.25, w_wp=0.2, w_v=0.05, w_j=0.3, w_c=0.15, w_vf=0.05,
                  jpos_diffw=[float(x) for x in np.round(np.linspace(0.5, 1.5, 24), 3)])
# (reward_v, observation kind of the next observation, body_diff_thresh, w_vf override)
REWARD_FLAVOURS = [(0, 2, 0.5, None), (1, 6, 0.2, None), (2, 5, 0.5, None), (2, 3, 0.2, 0.0), (3, 4, 0.5, None), (4, 0, 0.2, None), (5, 1, 0.5, None),
                   (0, "ball", 0.5, None)]
QUAT_KINDS = ["exact", "neg", "rot90", "rot179.9", "rot359.9", "scaled"]
REWARD_CASES = [f"quat_{k}" for k in QUAT_KINDS] + ["quat_mixed", "bd_0.5-", "bd_0.5+", "bd_0.2-", "bd_0.2+", "bd_eq0.5", "plain"]
BD_MARGIN = 1e-9


def reward_weights(rv, w_vf=None):
    w = dict(REWARD_W23 if rv >= 4 else REWARD_W)
    if w_vf is not None:
        w["w_vf"] = w_vf
    return w


def _target_quats(cur, kinds, rng):
    """cur (nb, 4): per body the expert quaternion that is `kind` away from the current one (cur (x) e^-1 = r^-1 for e = r (x) cur)."""
    out = np.empty_like(cur)
    for b, k in enumerate(kinds):
        ax = rng.normal(size=3)
        if k == "exact":
            out[b] = cur[b]
        elif k == "neg":
            out[b] = -cur[b]
        elif k == "scaled":
            out[b] = 1.001 * cur[b]
        else:
            out[b] = quaternion_multiply(axis_quat(float(k[3:]) * PI / 180, ax), cur[b])
    return out


def craft_reward_record(rec, case, st, prev_qpos, dt, jw, ball, seed):
    """Rewrites the non-qpos, non-qvel slots of the frame record `rec` (584,) relative to the post-step state `st`: every reward term gets an
    argument of order one, and `case` puts the quaternion targets / the termination distance where it says."""
    rng = np.random.default_rng(seed)
    nb = st["xpos"].shape[0] - 1
    cur_b = (E.get_body_quat_ball(st["qpos"]) if ball else E.get_body_quat(st["qpos"])).reshape(nb, 4)
    prev_b = E.get_body_quat_ball(prev_qpos) if ball else E.get_body_quat(prev_qpos)
    if case.startswith("quat_"):
        k = case[5:]
        kinds = [QUAT_KINDS[(b + 1) % len(QUAT_KINDS)] for b in range(nb)] if k == "mixed" else [k] * nb
    else:
        kinds = ["rot20"] * nb
    sl = lambda name: slice(FR[name][0], FR[name][0] + FR[name][1])  # noqa: E731
    rec[sl("bquat")] = _target_quats(cur_b, kinds, rng).ravel()
    rec[sl("wbquat")] = _target_quats(st["xquat"][1:], kinds[::-1], rng).ravel()
    rec[sl("bangvel")] = E.get_angvel_fd(prev_b, cur_b.ravel(), dt) + rng.normal(scale=1.0, size=3 * nb)
    rec[sl("ee_wpos")] = st["xpos"][E.EE_BODY_IDS].ravel() + rng.normal(scale=0.08, size=15)
    rec[sl("com")] = st["xipos"][1] + rng.normal(scale=0.03, size=3)
    rec[sl("body_com")] = st["xipos"][1:].ravel() + rng.normal(scale=0.03, size=3 * nb)
    disp = rng.normal(size=(nb, 3))
    disp /= np.linalg.norm(disp, axis=1, keepdims=True)
    if case == "bd_eq0.5":
        # termination distance EXACTLY 0.5, in exact arithmetic on either side: every weighted body (weight 1) is off by 0.5 along one axis, chosen so that
        # x - fl(x -+ 0.5) is +-0.5 without rounding; |d| = sqrt(0.25) = 0.5, the sum of twenty halves is 10 in any order, 10 / 20 = 0.5.  `>` is false here.
        wb = st["xpos"][1:].copy()
        for b in range(nb):
            pick = [(k, s) for k in range(3) for s in (0.5, -0.5) if st["xpos"][b + 1, k] - (st["xpos"][b + 1, k] - s) == s]
            k, s = pick[b % len(pick)]
            wb[b, k] = st["xpos"][b + 1, k] - s
        rec[sl("wbpos")] = wb.ravel()
    elif case.startswith("bd_"):
        thr, above = float(case[3:-1]), case.endswith("+")
        want = thr + (BD_MARGIN if above else -BD_MARGIN)
        scale = want
        for _ in range(6):  # every weighted body at the same weighted distance; two rounds of rescaling settle the mean to a few 1e-16
            rec[sl("wbpos")] = (st["xpos"][1:] + disp * scale).ravel()
            scale *= want / E.calc_body_diff(st["xpos"], rec[sl("wbpos")], jw)
    else:
        rec[sl("wbpos")] = (st["xpos"][1:] + disp * rng.uniform(0.01, 0.08, size=(nb, 1))).ravel()
    return rec


def oracle_reward(rv, st, prev_qpos, action, win, cur_t, dt, jw, w, ball=False, vf_dim=6, ndof=69):
    """-> [reward, six reward parts (the five-part flavours padded with 0), body_diff]."""
    ex = expert_of_window(win)
    prev_b = E.get_body_quat_ball(prev_qpos) if ball else E.get_body_quat(prev_qpos)
    q, xp, xq, xi = st["qpos"], st["xpos"], st["xquat"], st["xipos"]
    if rv >= 4:
        w23 = {k: v for k, v in w.items() if k != "jpos_diffw"}
        r, parts = E.world_rfc_implicit_v2_v3(rv == 5, q, xp, xq, xi, prev_b, action, ex, cur_t, 0, dt, w23, np.asarray(w["jpos_diffw"]), ndof=ndof, vf_dim=vf_dim)
    elif rv == 3:
        r, parts = E.world_rfc_mul_reward(True, q, xp, xi, prev_b, action, ex, cur_t, 0, dt, jw[1:], w, ndof=ndof)
    elif rv == 2:
        r, parts = E.world_rfc_mul_reward(False, q, xp, xi, prev_b, action, ex, cur_t, 0, dt, jw[1:], w, ndof=ndof, vf_dim=vf_dim, ball=ball)
    elif rv == 1:
        r, parts = E.world_rfc_explicit_reward(q, xp, xi, prev_b, action, ex, cur_t, 0, dt, jw[1:], w, ndof=ndof)
    else:
        r, parts = E.world_rfc_implicit_reward(q, xp, xi, prev_b, action, ex, cur_t, 0, dt, jw[1:], w, ndof=ndof, vf_dim=vf_dim, ball=ball)
    bd = E.calc_body_diff(xp, ex["wbpos"][E.expert_index(cur_t, 0, ex["len"])], jw)
    return np.r_[r, parts, np.zeros(6 - len(parts)), bd]


def reward_reference(rv, st, prev_qpos, action, win, cur_t, dt, jw, w, thresh, seed, check_side=True, **kw):
    def fn(q, xp, xq, xi, pq, act, wn):
        return oracle_reward(rv, dict(qpos=q, xpos=xp, xquat=xq, xipos=xi), pq, act, wn, cur_t, dt, jw, w, **kw)

    arrays = [st["qpos"], st["xpos"], st["xquat"], st["xipos"], prev_qpos, action, win]
    return measured_bar(fn, arrays, seed, side=(lambda *a: bool(fn(*a)[-1] > thresh)) if check_side else None)


def episode_schedule(length, trail, episode_len, steps):
    """Per control step: (cur_t, expert index, past the clip end, end flag, percent) -- humanoid_im.py:1213-1243."""
    out = []
    for t in range(1, steps + 1):
        out.append((t, E.expert_index(t, 0, length), t >= length, t >= episode_len or t >= length + trail - 1, t / (length - 1)))
    return out


def explicit_action(n, action_dim, seed, nu=69, n_vf=24 * 9):
    """Small joint targets; residual entries with a different value in each of a body's nine slots (contact point 0-2, force 3-5, torque 6-8)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(scale=0.05, size=(n, action_dim))
    k = np.arange(n_vf)
    a[:, nu:nu + n_vf] = 0.01 * (1 + k % 9) * np.where(k // 9 % 2 == 0, 1.0, -1.0) * (1 + 0.1 * np.arange(n)[:, None])
    return a
