"""Expected values for srt_temporal_accumulate's per-collider motion (tests/test_temporal_motion.py,
tests/test_gpu_temporal_motion.py), restated in numpy on top of tests/temporal_ref.py.  csrc/rt_denoise.h and
sightpy/_motion.py state the same definitions; nothing here reads them.

motion (rows, 12) float64: row m = (R row-major, t) of the collider with hit_id m maps a point of the current frame
to the same surface point of the previous frame.  For pixel p with id = hit_id_p:
    id < 0, id >= rows, or a NaN anywhere in the row: no history for p
    x'_k = ((R[k][0]*x_p.x + R[k][1]*x_p.y) + R[k][2]*x_p.z) + t[k];  n'_k = (R[k][0]*n_p.x + R[k][1]*n_p.y) + R[k][2]*n_p.z
    then temporal_ref.accumulate on guides whose position / normal are x' / n' (depth, hit_id, albedo as they are)
(A NaN in a row makes some x'_k NaN, so zc is NaN and fails zc > 0: the definition needs no separate rule for it.
Here such a pixel is given a hit_id no history pixel has, which refuses all its taps -- the same outcome, and the
margins temporal_ref.accumulate reports stay finite.)  motion None: temporal_ref.accumulate itself.
"""
import numpy as np

import temporal_ref as TR

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
NO_ID = -2  # a hit_id that no pixel of a history carries


def identity_rows(n):
    return np.tile(IDENTITY, (n, 1))


def transformed_guides(guides, motion):
    """The guides temporal_ref.accumulate takes in place of `guides` under `motion` (the module comment)."""
    motion = np.asarray(motion, dtype=np.float64).reshape(-1, 12)
    ids = np.asarray(guides["hit_id"]).reshape(-1)
    n = ids.size
    x = np.asarray(guides["position"], dtype=np.float64).reshape(3, n)
    nm = np.asarray(guides["normal"], dtype=np.float64).reshape(3, n)
    known = (ids >= 0) & (ids < len(motion))
    rows = motion[np.where(known, ids, 0)]  # (n, 12)
    known &= ~np.isnan(rows).any(axis=1)
    rows = np.where(known[:, None], rows, IDENTITY)
    R = lambda k, j: rows[:, 3 * k + j]
    x2 = np.stack([((R(k, 0) * x[0] + R(k, 1) * x[1]) + R(k, 2) * x[2]) + rows[:, 9 + k] for k in range(3)])
    n2 = np.stack([(R(k, 0) * nm[0] + R(k, 1) * nm[1]) + R(k, 2) * nm[2] for k in range(3)])
    # a background pixel keeps its zero normal: "ok" is decided on the untransformed guide
    bg = (nm == 0.0).all(axis=0)
    n2[:, bg] = 0.0
    return dict(guides, position=x2, normal=n2, hit_id=np.where(known | bg, ids, NO_ID).astype(np.int32))


def accumulate(A, B, guides, W, H, history=None, prev_cam=None, motion=None, **kw):
    """temporal_ref.accumulate with a motion table."""
    if motion is None or history is None:
        return TR.accumulate(A, B, guides, W, H, history=history, prev_cam=prev_cam, **kw)
    return TR.accumulate(A, B, transformed_guides(guides, motion), W, H, history=history, prev_cam=prev_cam, **kw)


# ---- motion rows from the scene's objects (centres and axes), independent of sightpy/_motion.py --------------
def _v(v):
    return np.array([float(v.x), float(v.y), float(v.z)])


def _unit(v):
    return v / np.sqrt(v @ v)


def snapshot(scene):
    """What object_motion needs of every collider of `scene`, copied (the objects change in place between frames):
    [(kind, size, origin (3,), frame (3, 3) with orthonormal columns fixed to the object)]."""
    out = []
    for c in scene.collider_list:
        kind = type(c).__name__
        if kind == "Sphere_Collider":
            out.append((kind, (float(c.radius),), _v(c.center), np.eye(3)))
        elif kind == "Plane_Collider":
            out.append((kind, (float(c.w), float(c.h)), _v(c.center), np.stack([_v(c.u_axis), _v(c.v_axis), _v(c.normal)], axis=1)))
        elif kind == "Cuboid_Collider":
            out.append((kind, (float(c.width), float(c.height), float(c.length)), _v(c.center),
                        np.stack([_v(c.ax_w), _v(c.ax_h), _v(c.ax_l)], axis=1)))
        elif kind == "Triangle_Collider":
            p1, p2, p3 = _v(c.p1), _v(c.p2), _v(c.p3)
            e1 = _unit(p2 - p1)
            nn = _unit(np.cross(p2 - p1, p3 - p1))
            size = tuple(float(np.sqrt(d @ d)) for d in (p2 - p1, p3 - p1, p3 - p2))
            out.append((kind, size, p1, np.stack([e1, np.cross(nn, e1), nn], axis=1)))
        else:
            out.append((kind, (), np.zeros(3), np.full((3, 3), np.nan)))
    return out


def object_motion(prev, cur):
    """(n, 12) rows from two snapshots: with orthonormal frames fixed to the object, a point o_cur + F_cur l is the
    point o_prev + F_prev l of the previous frame, so R = sum_k outer(F_prev[:, k], F_cur[:, k]) and
    t = o_prev - R o_cur.  Another kind or size at an index: a NaN row; another number of colliders: all NaN."""
    out = np.full((len(cur), 12), np.nan)
    if len(prev) != len(cur):
        return out
    for i, ((k0, s0, o0, F0), (k1, s1, o1, F1)) in enumerate(zip(prev, cur)):
        if k0 != k1 or not np.allclose(s0, s1, rtol=1e-9, atol=0.0):
            continue
        if np.array_equal(o0, o1) and np.array_equal(F0, F1):
            out[i] = IDENTITY
            continue
        R = sum(np.outer(F0[:, k], F1[:, k]) for k in range(3))
        out[i, :9], out[i, 9:] = R.reshape(9), o0 - R @ o1
    return out


def rotation_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def row_about(R, centre, shift=(0.0, 0.0, 0.0)):
    """The row of x -> R (x - centre) + centre + shift."""
    centre = np.asarray(centre, dtype=np.float64)
    return np.concatenate([R.reshape(9), centre - R @ centre + np.asarray(shift, dtype=np.float64)])


# ---- generators ----------------------------------------------------------------------------------------------
def moved_plane_guides(cam, W, H, rows, rng=None):
    """temporal_ref.plane_guides' scene (back wall id 0, slab id 1, tilted floor id 2) seen through `cam`, each
    plane moved to where `rows` (3, 12; current -> previous, no NaN) puts it: the previous frame's guides.  A ray
    O + s D meets the moved plane where R^T (O - t) + s R^T D meets the plane itself, and the extent of a plane is
    judged there; position and normal are reported in the moved frame."""
    n = W * H
    cw, ch = cam["cam_width"], cam["cam_height"]
    xs, ys = np.linspace(-cw / 2, cw / 2, W), np.linspace(ch / 2, -ch / 2, H)
    px, py = np.tile(xs, H), np.repeat(ys, W)
    fwd = cam["fwd_fd"] / cam["focal_distance"]
    D = cam["right"].reshape(3, 1) * px + cam["up"].reshape(3, 1) * py + fwd.reshape(3, 1)
    D = D / np.sqrt(TR._sq(D))
    O = cam["look_from"].reshape(3, 1)
    top = 0.25 * ch * 6.0 if H > 1 else np.inf
    tilt = 0.3
    planes = ((np.array([0.0, 0.0, -6.0]), np.array([0.0, 0.0, 1.0]), lambda P: P[1] < top),
              (np.array([0.0, 0.0, -4.0]), np.array([0.0, 0.0, 1.0]),
               lambda P: (P[0] > 0.05 * cw * 4) & (P[0] < 0.35 * cw * 4) & (P[1] < 0.1 * ch * 4)),
              (np.array([0.0, -0.2 * ch * 6.0, -6.0]), np.array([0.0, np.cos(tilt), np.sin(tilt)]), lambda P: P[2] > -6.0))
    best = np.full(n, 1.0e39)
    g = {"hit_id": np.full(n, -1, dtype=np.int32), "depth": np.full(n, 1.0e39), "position": np.zeros((3, n)),
         "normal": np.zeros((3, n)), "albedo": np.zeros((3, n))}
    for i, (p0, nrm, inside) in enumerate(planes):
        R, t = rows[i, :9].reshape(3, 3), rows[i, 9:].reshape(3, 1)
        Ol, Dl = R.T @ (O - t), R.T @ D
        with np.errstate(all="ignore"):
            s = TR._dot(p0.reshape(3, 1) - Ol, nrm.reshape(3, 1)) / TR._dot(Dl, nrm.reshape(3, 1))
        hit = np.isfinite(s) & (s > 0.0) & (s < best) & inside(Ol + Dl * s)
        best = np.where(hit, s, best)
        g["hit_id"][hit] = i
        g["depth"][hit] = s[hit]
        g["position"][:, hit] = (O + D * s)[:, hit]
        facing = np.where(TR._dot(Dl, nrm.reshape(3, 1)) < 0.0, 1.0, -1.0)
        g["normal"][:, hit] = ((R @ nrm).reshape(3, 1) * facing)[:, hit]
    seen = g["hit_id"] >= 0
    alb = 0.5 + 0.3 * np.stack([np.sin(g["position"][0] * 3.0), np.cos(g["position"][1] * 5.0), np.sin(g["position"][2])])
    if rng is not None:
        alb = alb + 0.02 * rng.standard_normal((3, n))
    g["albedo"][:, seen] = np.clip(alb, 0.0, 1.0)[:, seen]
    return g


def moving_sequence(W, H, seed):
    """temporal_ref.random_sequence with moving objects: the back wall stands still (an identity row), the slab was
    turned by 5 degrees about the vertical axis through (0.8, 0, -4) and shifted in the previous frame, the floor
    moved too but its row is NaN (so none of its pixels may find history).  The previous guides come from the moved
    planes through a slightly different camera; the history has random_sequence's blocks of hist_len 0, another
    hist_hit_id, another hist_normal and hist_position off the plane, the half-frames an inf and a nan.  No value
    that the definition compares lies within MARGIN of its threshold, with either flag.
    random_sequence's keys and "motion" (3, 12)."""
    rng = np.random.default_rng(seed)
    n = W * H
    cam = TR.make_camera(W, H)
    prev_cam = TR.make_camera(W, H, look_from=(0.25, 0.05, 0.1), yaw=0.01)
    slab = row_about(rotation_y(5.0), (0.8, 0.0, -4.0), shift=(0.11, -0.03, 0.15))
    floor = row_about(rotation_y(2.0), (0.0, 0.0, -5.0), shift=(0.05, 0.0, 0.02))
    guides = TR.plane_guides(cam, W, H, rng)
    prev = moved_plane_guides(prev_cam, W, H, np.stack([IDENTITY, slab, floor]), rng)
    motion = np.stack([IDENTITY, slab, np.full(12, np.nan)])
    A, B = 0.5 + 0.4 * rng.random((3, n)), 0.5 + 0.4 * rng.random((3, n))
    hist = {"a": 0.5 + 0.4 * rng.random((3, n)), "b": 0.5 + 0.4 * rng.random((3, n)),
            "len": rng.integers(1, 7, n).astype(np.float64), "hit_id": prev["hit_id"].copy(),
            "position": prev["position"].copy(), "normal": prev["normal"].copy()}
    hist["len"][prev["hit_id"] < 0] = 0.0
    seq = {"A": A, "B": B, "guides": guides, "history": hist, "prev_cam": prev_cam, "cam": cam, "inf": None, "nan": None,
           "motion": motion}
    if n > 1:
        yy, xx = (v.reshape(n) for v in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
        # blocks over the columns where the previous frame shows the slab (and the wall around it)
        block = lambda lo, hi: (xx >= int(lo * W)) & (xx < max(int(hi * W), int(lo * W) + 1))
        hist["len"][block(0.0, 0.1)] = 0.0
        hist["hit_id"][block(0.55, 0.6)] = 7
        hist["normal"][:, block(0.6, 0.65)] = np.array([[1.0], [0.0], [0.0]])
        shifted = block(0.65, 0.7)
        hist["position"][:, shifted] += 0.5 * hist["normal"][:, shifted]
        okpix = np.flatnonzero((guides["hit_id"] >= 0) & block(0.8, 1.0))
        assert okpix.size > 1 and (guides["hit_id"] < 0).any()
        seq["inf"], seq["nan"] = int(okpix[0]), int(okpix[-1])
        A[1, seq["inf"]] = np.inf
        B[2, seq["nan"]] = np.nan
    for demodulate in (False, True):
        info = {}
        accumulate(A, B, guides, W, H, history=hist, prev_cam=prev_cam, motion=motion, demodulate=demodulate, info=info)
        assert info["margin"] > TR.MARGIN, (W, H, seed, info["margin"])
    return seq


def turned_plane(W=17, H=9, deg=30.0, z=5.0):
    """A wall through the view axis facing the camera at depth z (the current frame, id 0) that stood turned by
    `deg` about the vertical axis through its centre in the previous frame, both seen by make_camera(W, H).
    (guides, the previous frame's guides, cam, the row)."""
    n = W * H
    cam = TR.make_camera(W, H)
    cw, ch = cam["cam_width"], cam["cam_height"]
    xs, ys = np.linspace(-cw / 2, cw / 2, W), np.linspace(ch / 2, -ch / 2, H)
    px, py = np.tile(xs, H), np.repeat(ys, W)
    P = np.stack([px * z, py * z, np.full(n, -z)])
    guides = {"hit_id": np.zeros(n, dtype=np.int32), "depth": np.sqrt(TR._sq(P)), "position": P,
              "normal": np.stack([np.zeros(n), np.zeros(n), np.ones(n)]), "albedo": np.full((3, n), 0.5)}
    R = rotation_y(deg)
    c = np.array([0.0, 0.0, -z])
    row = row_about(R, c)
    # the previous frame: the rays of the same camera against the plane through c with normal R (0, 0, 1)
    nq = R @ np.array([0.0, 0.0, 1.0])
    D = np.stack([px, py, np.full(n, -1.0)])
    s = (c @ nq) / (nq.reshape(1, 3) @ D).reshape(n)
    assert (s > 0.0).all()
    Q = D * s
    prev = {"hit_id": np.zeros(n, dtype=np.int32), "depth": np.sqrt(TR._sq(Q)), "position": Q,
            "normal": np.repeat(nq.reshape(3, 1), n, axis=1), "albedo": np.full((3, n), 0.5)}
    return guides, prev, cam, row


# ---- the checks both suites run; `run` has accumulate's signature (without `info`) and result -----------------
def check_exact_shift_by_motion(run, columns):
    """shifted_plane's wall, the same camera for both frames, and id 0's row R = I, t = (columns*z*cw/(W-1), 0, 0):
    x' lies `columns` pixel columns further along `right`, which is what a previous camera -columns columns along
    `right` sees -- temporal_ref.check_exact_shift's expectations for that camera (the history of column
    c + columns blended at alpha 1/2 within 1e-9, len 2; the column whose x' left the image has len 1 and
    out_a == A bit for bit).  Without the table the same call blends column c itself."""
    W, H, z = 9, 4, 5.0
    cam = TR.make_camera(W, H)
    row = IDENTITY.copy()
    row[9] = columns * z * cam["cam_width"] / (W - 1)
    seen = {}

    def with_row(A, B, guides, W, H, history=None, prev_cam=None, **kw):
        seen.update(A=A, B=B, history=history)
        seen["plain"] = run(A, B, guides, W, H, history=history, prev_cam=cam, motion=None, **kw)
        seen["moved"] = run(A, B, guides, W, H, history=history, prev_cam=cam, motion=row.reshape(1, 12), **kw)
        return seen["moved"]

    TR.check_exact_shift(with_row, -columns)
    plain, hist = seen["plain"], seen["history"]
    for k, cur in (("a", seen["A"]), ("b", seen["B"])):
        dev = np.abs(plain[k] - (hist[k] + 0.5 * (cur - hist[k]))).max()
        print("no table:", k, "largest deviation from column c itself", dev)
        assert dev <= 1e-9
        assert np.abs(plain[k] - seen["moved"][k]).max() > 1e-3
    assert (plain["len"] == 2.0).all()


def check_rotation(run):
    """turned_plane: |n_p - n_q|^2 = 2 - 2 cos 30 = 0.268 > normal_max, so without the row no pixel finds history;
    with it every pixel whose x' projects inside the image does (x' lies on the previous plane, all four taps are
    inside and agree), and the result is the restatement's."""
    from denoise_ref import close

    W, H = 17, 9
    n = W * H
    guides, prev, cam, row = turned_plane(W, H)
    rng = np.random.default_rng(17)
    A, B = rng.random((3, n)), rng.random((3, n))
    hist = {"a": rng.random((3, n)), "b": rng.random((3, n)), "len": rng.integers(1, 5, n).astype(np.float64),
            "hit_id": prev["hit_id"], "position": prev["position"], "normal": prev["normal"]}
    dn2 = TR._sq(guides["normal"][:, :1] - prev["normal"][:, :1])[0]
    assert dn2 > 0.25
    motion = row.reshape(1, 12)
    info = {}
    ref = accumulate(A, B, guides, W, H, history=hist, prev_cam=cam, motion=motion, info=info)
    assert info["margin"] > TR.MARGIN
    got = run(A, B, guides, W, H, history=hist, prev_cam=cam, motion=motion)
    for k in TR.OUTPUTS:
        close(got[k], ref[k])
    _, fx, fy = TR.project(transformed_guides(guides, motion)["position"], cam, W, H)
    inside = (fx >= 0.0) & (fx <= W - 1.0) & (fy >= 0.0) & (fy <= H - 1.0)
    print("rotation: pixels whose x' projects inside the image", int(inside.sum()), "of", n)
    assert inside.sum() > n // 3 and (~inside).any()
    assert (got["len"][inside] > 1.0).all() and np.array_equal(got["len"] > 1.0, info["has"])
    assert np.abs(got["a"][:, inside] - A[:, inside]).max() > 1e-3
    plain = run(A, B, guides, W, H, history=hist, prev_cam=cam, motion=None)
    assert (plain["len"] == 1.0).all() and TR.same_bits(plain["a"], A) and TR.same_bits(plain["b"], B)


def check_identity_and_unknown_rows(run):
    """random_sequence(70, 9, 5): an all-identity table changes nothing; id 2's row NaN, or a table of two rows,
    leaves id 2's pixels without history and the other ids' as they are."""
    W, H = 70, 9
    s = TR.random_sequence(W, H, 5)
    A, B, guides = s["A"], s["B"], s["guides"]
    call = lambda motion: run(A, B, guides, W, H, history=s["history"], prev_cam=s["prev_cam"], demodulate=True, motion=motion)
    plain = call(None)
    ident = call(identity_rows(3))
    for k in TR.OUTPUTS:
        assert np.array_equal(ident[k], plain[k], equal_nan=True), k
    ids = guides["hit_id"]
    two = ids == 2
    ok = np.isfinite(A).all(axis=0) & np.isfinite(B).all(axis=0)
    assert (plain["len"][two] > 1.0).any() and (plain["len"][~two] > 1.0).any()
    unknown = identity_rows(3)
    unknown[2, 4] = np.nan
    for motion in (unknown, identity_rows(2)):
        got = call(motion)
        assert (got["len"][two & ok] == 1.0).all() and not got["len"][two & ~ok].any()
        assert TR.same_bits(got["a"][:, two], A[:, two]) and TR.same_bits(got["b"][:, two], B[:, two])
        for k in TR.OUTPUTS:
            assert np.array_equal(got[k][..., ~two], plain[k][..., ~two], equal_nan=True), k


def check_against_restatement(run, W, H, demodulate):
    """`run` on moving_sequence(W, H) against the restatement; the slab keeps history only by its row."""
    from denoise_ref import close

    s = moving_sequence(W, H, 10 * W + H)
    A, B, guides = s["A"], s["B"], s["guides"]
    kw = dict(history=s["history"], prev_cam=s["prev_cam"], demodulate=demodulate)
    info, info0 = {}, {}
    ref = accumulate(A, B, guides, W, H, motion=s["motion"], info=info, **kw)
    got = run(A, B, guides, W, H, motion=s["motion"], **kw)
    worst = 0.0
    for k in TR.OUTPUTS:
        close(got[k], ref[k])
        sel = np.isfinite(ref[k]) & (ref[k] != 0.0)
        if sel.any():
            worst = max(worst, float((np.abs(got[k][sel] - ref[k][sel]) / np.abs(ref[k][sel])).max()))
    print("motion against the restatement", (W, H), "demodulate", demodulate, "largest relative deviation %.3g" % worst)
    has, ids = info["has"], guides["hit_id"]
    floor = ids == 2
    assert not has[floor].any()
    assert TR.same_bits(got["a"][:, floor], A[:, floor]) and TR.same_bits(got["b"][:, floor], B[:, floor])
    if W * H >= 70 * 9:
        accumulate(A, B, guides, W, H, info=info0, **kw)
        # (an image wide enough to show the slab in both frames) every kind of pixel: history found -- by the identity
        # row, and by the slab's row alone -- and refused
        assert has[ids == 0].any() and has[ids == 1].any() and (~has[ids == 1]).any()
        assert (has & ~info0["has"] & (ids == 1)).any()
    return got, ref, info
