"""Toy sequences for the surface metrics (penetration, skate, float, contact count), shared by tests/test_surface_metrics_cpu.py (the host probe) and
tests/test_gpu_surface_metrics.py (the kernel): 2 bodies, every vertex count around the wave width, sequences of 1, 2 and 5 rows, and what
uhc_amd.smpllib.smpl_eval's host functions give for them.  Random cases keep every vertex at least 1e-6 m from the floor (asserted when a case is built), so
that no comparison hangs on the last bit of a height; the vertex that lies EXACTLY on the floor is built from dyadic numbers and exact rotations."""
import warnings

import numpy as np

N_BODY = 2
VERTS = (1, 63, 64, 65, 130)
ROWS = (1, 2, 5)
KINDS = ("mixed", "clear", "sunk", "exact", "radius", "floor", "models", "nan")
SENTINEL = -7.0
NAMES = ("pentration", "skate", "float", "contact")


def _unit_quats(rng, shape):
    q = rng.normal(size=shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_case(kind, V, T, seed=0):
    """-> dict(kind, V, T, vert [n_models][V][3], vert_body [V] int32, vert_radius [V] or None, pos [T][2][3], quat [T][2][4], floor_z, model, nan_row)"""
    rng = np.random.default_rng([KINDS.index(kind), V, T, seed])
    c = dict(kind=kind, V=V, T=T, floor_z=0.0, model=0, vert_radius=None, nan_row=None)
    body = rng.integers(0, N_BODY, size=V).astype(np.int32)
    if V >= 2:
        body[0], body[-1] = 0, 1
    c["vert_body"] = body
    if kind == "exact":
        # dyadic coordinates, rotations whose matrices are exactly 0 / +-1 (quaternions with |q|^2 = 1 or 2: the identity, half turns, quarter turns)
        turns = np.array([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 0, 0], [1, -1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
        vert = rng.integers(-16, 17, size=(1, V, 3)) / 64.0
        quat = turns[rng.integers(0, len(turns), size=(T, N_BODY))]
        pos = rng.integers(-64, 65, size=(T, N_BODY, 3)) / 64.0
        c.update(vert=vert, quat=quat, pos=pos)
        # vertex 0 (of body 0) onto the floor in every row: the body's height is minus the vertex's rotated height, exactly
        from uhc_amd.smpllib.smpl_eval import hull_vertices
        pos[:, 0, 2] = 0.0
        w = hull_vertices((vert[0], body, np.zeros(V)), pos, quat)
        pos[:, 0, 2] = -w[:, 0, 2]
        return c
    n_models = 2 if kind == "models" else 1
    c["vert"] = rng.uniform(-0.3, 0.3, size=(n_models, V, 3))
    c["model"] = n_models - 1
    c["quat"] = _unit_quats(rng, (T, N_BODY))
    pos = rng.uniform(-1.0, 1.0, size=(T, N_BODY, 3))
    pos[:, :, 2] = {"clear": 1.0, "sunk": -1.0}.get(kind, 0.0) + rng.uniform(-0.1, 0.1, size=(T, N_BODY))
    if kind == "radius":
        c["vert_radius"] = rng.uniform(0.01, 0.05, size=V)
    if kind == "floor":
        c["floor_z"] = 0.37
        pos[:, :, 2] += 0.37
    c["pos"] = pos
    assert_clear_of_the_floor(c)
    if kind == "nan":
        c["nan_row"] = T // 2
        pos[T // 2, 1, 2] = np.nan if T != 5 else np.inf
    return c


def tables(c, model=None):
    return c["vert"][c["model"] if model is None else model], c["vert_body"], c["vert_radius"] if c["vert_radius"] is not None else np.zeros(c["V"])


def heights(c):
    from uhc_amd.smpllib.smpl_eval import hull_vertices
    return hull_vertices(tables(c), c["pos"], c["quat"])[:, :, 2] - c["floor_z"]


def assert_clear_of_the_floor(c, margin=1e-6):
    h = heights(c)
    assert np.abs(h).min() > margin, (c["kind"], c["V"], c["T"], float(np.abs(h).min()))


def expected(c):
    """(rows [T][4], means [4], bad) from the host functions: SENTINEL where nothing is written (the skate of the last row); a row with a non-finite
    pose is NaN in its four values and in the skate of the row before it, and counts in bad"""
    from uhc_amd.smpllib import smpl_eval as E
    T = c["T"]
    pos, quat = c["pos"].copy(), c["quat"].copy()
    k = c["nan_row"]
    if k is not None:
        pos[k] = np.nan_to_num(pos[k], nan=0.0, posinf=0.0, neginf=0.0)  # (any finite stand-in: the row's values are overwritten below)
    vert = E.hull_vertices(tables(c), pos, quat)
    info = {"floor_z": c["floor_z"]}
    rows = np.full((T, 4), SENTINEL)
    rows[:, 0] = E.compute_penetration(vert, info)
    rows[:T - 1, 1] = E.compute_skate(vert, info)
    rows[:, 2] = E.compute_float(vert, info)
    rows[:, 3] = E.compute_contact(vert, info)
    if k is not None:
        rows[k, [0, 2, 3]] = np.nan
        if k + 1 < T:
            rows[k, 1] = np.nan
        if k >= 1:
            rows[k - 1, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (np.mean of an empty array warns and gives the NaN asked for)
        means = np.array([np.mean(rows[:T - (1 if j == 1 else 0), j]) for j in range(4)])
    return rows, means, 0 if k is None else 1


def all_cases():
    return [make_case(kind, V, T) for kind in KINDS for V in VERTS for T in ROWS]


def assert_rows_match(got_rows, got_means, exp_rows, exp_means, what, atol=1e-9):
    """1e-9 mm absolute (coordinates <= 2 m, sums of <= 2 000 terms: float64 leaves a mean below 1e-12 mm); NaN where NaN is expected; the contact count
    exactly; untouched slots still hold the sentinel"""
    np.testing.assert_allclose(got_rows, exp_rows, atol=atol, rtol=0, equal_nan=True, err_msg=str(what))
    np.testing.assert_array_equal(got_rows[:, 3], exp_rows[:, 3], err_msg=str(what))
    np.testing.assert_array_equal(got_rows == SENTINEL, exp_rows == SENTINEL, err_msg=str(what))
    np.testing.assert_allclose(got_means, exp_means, atol=atol, rtol=0, equal_nan=True, err_msg=str(what))
