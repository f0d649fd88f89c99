"""Expected values for the temporal accumulation of half-frames (tests/test_temporal.py,
tests/test_gpu_temporal.py), restated in numpy.  csrc/rt_denoise.h states the same definition; nothing here reads
it.  Everything is float64, in the order written; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and
|v|^2 = (v.x*v.x + v.y*v.y) + v.z*v.z.

Pixel p of the current frame: half-frames A, B, guides hit_id_p, x_p (position), n_p (normal), albedo, t_p (depth).
The previous call left hist_a, hist_b, hist_len and that frame's hit_id / position / normal; primes mark the previous
frame's camera.  history None: a first frame.
    ok = p is not background (n_p != 0) and A, B are finite
    d = max(albedo, 1e-3) per channel with `demodulate`, else 1;  uA = A/d, uB = B/d
    not ok:  out_a = A, out_b = B, out_hist_a = A, out_hist_b = B, out_len = 0
    e = x_p - look_from';  fwd' = fwd_fd' / focal_distance';  zc = dot(e, fwd')
    xc = dot(e, right') / zc;  yc = dot(e, up') / zc
    fx = ((xc + cw'/2) / cw') * (W-1) if W > 1 else 0;  fy = ((ch'/2 - yc) / ch') * (H-1) if H > 1 else 0
    no history unless zc > 0, -1 < fx < W and -1 < fy < H
    x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0
    taps, in this order: (y0, x0) w = (1-ax)*(1-ay); (y0, x0+1) w = ax*(1-ay); (y0+1, x0) w = (1-ax)*ay;
        (y0+1, x0+1) w = ax*ay
    tap q is valid when it is inside the image, w > 0, hist_len_q >= 1, hist_hit_id_q == hit_id_p,
        |n_p - n_q|^2 <= normal_max and |dot(n_p, x_q - x_p)| / t_p <= plane_max
    sw = sum(w) over the valid taps; history exists when sw >= 0.01
    hA = sum(w * hist_a_q) / sw, hB likewise, L = sum(w * hist_len_q) / sw
    with history:     N = min(L + 1, max_history), alpha = 1/N, uA' = hA + alpha*(uA - hA), uB' likewise
                      out_len = N, out_hist_a/b = uA'/uB', out_a/b = uA'*d / uB'*d
    without history:  out_a = A, out_b = B, out_hist_a/b = uA/uB, out_len = 1
"""
import functools

import numpy as np

DEFAULTS = {"max_history": 32, "normal_max": 0.1, "plane_max": 0.02}
SW_MIN = 0.01
OUTPUTS = ("a", "b", "hist_a", "hist_b", "len")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sq(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def camera_dict(cam):
    """The scalars of a sightpy Camera that the projection reads (srt_camera's)."""
    f3 = lambda v: np.array([float(v.x), float(v.y), float(v.z)])
    return {"look_from": f3(cam.look_from), "right": f3(cam.cameraRight), "up": f3(cam.cameraUp),
            "fwd_fd": f3(cam.cameraFwd * cam.focal_distance), "focal_distance": float(cam.focal_distance),
            "cam_width": float(cam.camera_width), "cam_height": float(cam.camera_height)}


def project(x, cam, W, H):
    """(zc, fx, fy) of the points x (3, n) in the camera `cam` (a camera_dict)."""
    col = lambda k: np.asarray(cam[k], dtype=np.float64).reshape(3, 1)
    with np.errstate(all="ignore"):
        e = x - col("look_from")
        fwd = col("fwd_fd") / float(cam["focal_distance"])
        zc = _dot(e, fwd)
        xc = _dot(e, col("right")) / zc
        yc = _dot(e, col("up")) / zc
        cw, ch = float(cam["cam_width"]), float(cam["cam_height"])
        fx = ((xc + cw / 2.0) / cw) * float(W - 1) if W > 1 else np.zeros_like(zc)
        fy = ((ch / 2.0 - yc) / ch) * float(H - 1) if H > 1 else np.zeros_like(zc)
    return zc, fx, fy


def accumulate(A, B, guides, W, H, history=None, prev_cam=None, demodulate=False, max_history=DEFAULTS["max_history"],
               normal_max=DEFAULTS["normal_max"], plane_max=DEFAULTS["plane_max"], info=None):
    """{"a", "b", "hist_a", "hist_b" (3, n), "len" (n,)}.  `history`: None, or {"a", "b", "len", "hit_id", "position",
    "normal"} of the previous frame with `prev_cam` its camera_dict.  `info` (a dict) receives "has" (n,) -- the
    pixels that found history -- and "margin", the smallest distance of a value that was compared from its threshold
    (normal_max, plane_max, sw = 0.01, the fx / fy bounds, zc = 0)."""
    n = W * H
    A = np.array(A, dtype=np.float64).reshape(3, n)
    B = np.array(B, dtype=np.float64).reshape(3, n)
    nm = np.asarray(guides["normal"], dtype=np.float64).reshape(3, n)
    bg = (nm[0] == 0.0) & (nm[1] == 0.0) & (nm[2] == 0.0)
    ok = ~bg & np.isfinite(A).all(axis=0) & np.isfinite(B).all(axis=0)
    with np.errstate(all="ignore"):
        d = np.maximum(np.asarray(guides["albedo"], dtype=np.float64).reshape(3, n), 1e-3) if demodulate else None
        uA = np.where(ok, A / d, A) if demodulate else A
        uB = np.where(ok, B / d, B) if demodulate else B
    out = {"a": A.copy(), "b": B.copy(), "hist_a": uA.copy(), "hist_b": uB.copy(), "len": np.where(ok, 1.0, 0.0)}
    if info is not None:
        info["has"], info["margin"] = np.zeros(n, dtype=bool), np.inf
    if history is None:
        return out
    xp = np.asarray(guides["position"], dtype=np.float64).reshape(3, n)
    tp = np.asarray(guides["depth"], dtype=np.float64).reshape(n)
    ids = np.asarray(guides["hit_id"]).reshape(n)
    ha = np.asarray(history["a"], dtype=np.float64).reshape(3, n)
    hb = np.asarray(history["b"], dtype=np.float64).reshape(3, n)
    hl = np.asarray(history["len"], dtype=np.float64).reshape(n)
    hid = np.asarray(history["hit_id"]).reshape(n)
    hx = np.asarray(history["position"], dtype=np.float64).reshape(3, n)
    hn = np.asarray(history["normal"], dtype=np.float64).reshape(3, n)
    zc, fx, fy = project(xp, prev_cam, W, H)
    margins = []
    with np.errstate(all="ignore"):
        vis = ok & (zc > 0.0) & (fx > -1.0) & (fx < float(W)) & (fy > -1.0) & (fy < float(H))
        front = ok & (zc > 0.0)
        margins += [np.abs(zc[ok]), np.abs(fx[front] + 1.0), np.abs(fx[front] - W), np.abs(fy[front] + 1.0),
                    np.abs(fy[front] - H)]
        fxs, fys = np.where(vis, fx, 0.0), np.where(vis, fy, 0.0)
        xf, yf = np.floor(fxs), np.floor(fys)
        ax, ay = fxs - xf, fys - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        wts = ((1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay)
        sw, L = np.zeros(n), np.zeros(n)
        hA, hB = np.zeros((3, n)), np.zeros((3, n))
        tried = np.zeros(n, dtype=bool)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            w = wts[k]
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            q = np.clip(qy, 0, H - 1) * W + np.clip(qx, 0, W - 1)
            lq = hl[q]
            cand = vis & inside & (w > 0.0) & (lq >= 1.0) & (hid[q] == ids)
            dn2 = _sq(nm - hn[:, q])
            pl = np.abs(_dot(nm, hx[:, q] - xp)) / tp
            margins += [np.abs(dn2[cand] - normal_max), np.abs(pl[cand & (dn2 <= normal_max)] - plane_max)]
            valid = cand & (dn2 <= normal_max) & (pl <= plane_max)
            tried |= valid
            sw = sw + np.where(valid, w, 0.0)
            hA = hA + np.where(valid, ha[:, q] * w, 0.0)
            hB = hB + np.where(valid, hb[:, q] * w, 0.0)
            L = L + np.where(valid, w * lq, 0.0)
        margins.append(np.abs(sw[tried] - SW_MIN))
        has = vis & (sw >= SW_MIN)
        hA, hB, L = hA / sw, hB / sw, L / sw
        N = np.where(L + 1.0 < float(max_history), L + 1.0, float(max_history))
        alpha = 1.0 / N
        uA2 = hA + (uA - hA) * alpha
        uB2 = hB + (uB - hB) * alpha
        out["hist_a"] = np.where(has, uA2, uA)
        out["hist_b"] = np.where(has, uB2, uB)
        out["a"] = np.where(has, uA2 * d if demodulate else uA2, A)
        out["b"] = np.where(has, uB2 * d if demodulate else uB2, B)
        out["len"] = np.where(has, N, out["len"])
    if info is not None:
        info["has"] = has
        info["margin"] = min([float(m.min()) for m in margins if m.size] + [np.inf])
    return out


def next_history(out, guides):
    """What the next call takes as `history`: this call's results with this frame's guides."""
    return {"a": out["hist_a"], "b": out["hist_b"], "len": out["len"], "hit_id": guides["hit_id"],
            "position": guides["position"], "normal": guides["normal"]}


# ---- what the CPU and the GPU suite share ---------------------------------------------------------------
MARGIN = 1e-9


def make_camera(W, H, look_from=(0.0, 0.0, 0.0), yaw=0.0):
    """A camera looking down -z (turned by `yaw` about y), image plane 1.0 wide, focal distance 1.5."""
    cw = 1.0
    return {"look_from": np.array(look_from, dtype=np.float64), "right": np.array([np.cos(yaw), 0.0, -np.sin(yaw)]),
            "up": np.array([0.0, 1.0, 0.0]), "fwd_fd": np.array([-np.sin(yaw), 0.0, -np.cos(yaw)]) * 1.5,
            "focal_distance": 1.5, "cam_width": cw, "cam_height": cw * H / W}




def plane_guides(cam, W, H, rng=None):
    """The guides of a small analytic scene seen through `cam`: a back wall z = -6 (id 0) that ends above
    y = 0.25 * cam_height * 6 when H > 1 (the rows above it are background), a slab z = -4 over part of the image
    (id 1) and a tilted floor (id 2).  Albedo: smooth, with noise from `rng`."""
    n = W * H
    cw, ch = cam["cam_width"], cam["cam_height"]
    xs, ys = np.linspace(-cw / 2, cw / 2, W), np.linspace(ch / 2, -ch / 2, H)
    px, py = np.tile(xs, H), np.repeat(ys, W)
    fwd = cam["fwd_fd"] / cam["focal_distance"]
    D = cam["right"].reshape(3, 1) * px + cam["up"].reshape(3, 1) * py + fwd.reshape(3, 1)
    D = D / np.sqrt(_sq(D))
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
        with np.errstate(all="ignore"):
            t = _dot(p0.reshape(3, 1) - O, nrm.reshape(3, 1)) / _dot(D, nrm.reshape(3, 1))
        P = O + D * t
        hit = np.isfinite(t) & (t > 0.0) & (t < best) & inside(P)
        best = np.where(hit, t, best)
        g["hit_id"][hit] = i
        g["depth"][hit] = t[hit]
        g["position"][:, hit] = P[:, hit]
        facing = np.where(_dot(D, nrm.reshape(3, 1)) < 0.0, 1.0, -1.0)
        g["normal"][:, hit] = (nrm.reshape(3, 1) * facing)[:, hit]
    seen = g["hit_id"] >= 0
    alb = 0.5 + 0.3 * np.stack([np.sin(g["position"][0] * 3.0), np.cos(g["position"][1] * 5.0), np.sin(g["position"][2])])
    if rng is not None:
        alb = alb + 0.02 * rng.standard_normal((3, n))
    g["albedo"][:, seen] = np.clip(alb, 0.0, 1.0)[:, seen]
    return g


def random_sequence(W, H, seed):
    """A previous and a current frame of plane_guides' scene from two slightly different cameras, random
    half-frames and a random history with lengths 1..6, and among them (frames of more than one pixel): background
    pixels, an inf and a nan colour, a block of hist_len 0, a block of another hist_hit_id, a block of another
    hist_normal and a block of hist_position off the plane.  No value that the definition compares lies within
    MARGIN of its threshold, with either flag.
    {"A", "B", "guides", "history", "prev_cam", "cam", "inf", "nan" (pixel indices or None)}."""
    rng = np.random.default_rng(seed)
    n = W * H
    cam = make_camera(W, H)
    prev_cam = make_camera(W, H, look_from=(0.25, 0.05, 0.1), yaw=0.01)
    guides, prev = plane_guides(cam, W, H, rng), plane_guides(prev_cam, W, H, rng)
    A, B = 0.5 + 0.4 * rng.random((3, n)), 0.5 + 0.4 * rng.random((3, n))
    hist = {"a": 0.5 + 0.4 * rng.random((3, n)), "b": 0.5 + 0.4 * rng.random((3, n)),
            "len": rng.integers(1, 7, n).astype(np.float64), "hit_id": prev["hit_id"].copy(),
            "position": prev["position"].copy(), "normal": prev["normal"].copy()}
    prev_bg = prev["hit_id"] < 0
    hist["len"][prev_bg] = 0.0  # (what a call leaves on background pixels)
    seq = {"A": A, "B": B, "guides": guides, "history": hist, "prev_cam": prev_cam, "cam": cam, "inf": None, "nan": None}
    if n > 1:
        yy, xx = (v.reshape(n) for v in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
        low = yy >= (2 * H) // 3  # the bottom rows: the floor, seen by both cameras
        block = lambda lo, hi: low & (xx >= int(lo * W)) & (xx < max(int(hi * W), int(lo * W) + 1))
        hist["len"][block(0.0, 0.15)] = 0.0
        hist["hit_id"][block(0.2, 0.35)] = 7
        hist["normal"][:, block(0.4, 0.55)] = np.array([[1.0], [0.0], [0.0]])
        shifted = block(0.6, 0.75)
        hist["position"][:, shifted] += 0.5 * hist["normal"][:, shifted]
        okpix = np.flatnonzero((guides["hit_id"] >= 0) & block(0.8, 1.0))
        above = np.flatnonzero((guides["hit_id"] >= 0) & ~low)
        assert okpix.size and above.size and (guides["hit_id"] < 0).any()
        seq["inf"], seq["nan"] = int(okpix[0]), int(above[-1])
        A[1, seq["inf"]] = np.inf
        B[2, seq["nan"]] = np.nan
    for demodulate in (False, True):
        info = {}
        accumulate(A, B, guides, W, H, history=hist, prev_cam=prev_cam, demodulate=demodulate, info=info)
        assert info["margin"] > MARGIN, (W, H, seed, info["margin"])
    return seq


def shifted_plane(W, H, columns, z=5.0):
    """A wall facing the camera at depth z and a previous camera `columns` pixel columns further along `right`: the
    current pixel (r, c) then sees what the previous frame saw in column c - columns.  (guides, prev_cam)."""
    n = W * H
    cam = make_camera(W, H)
    cw, ch = cam["cam_width"], cam["cam_height"]
    xs, ys = np.linspace(-cw / 2, cw / 2, W), np.linspace(ch / 2, -ch / 2, H)
    P = np.stack([np.tile(xs, H) * z, np.repeat(ys, W) * z, np.full(n, -z)])
    guides = {"hit_id": np.zeros(n, dtype=np.int32), "depth": np.sqrt(_sq(P)), "position": P,
              "normal": np.stack([np.zeros(n), np.zeros(n), np.ones(n)]), "albedo": np.full((3, n), 0.5)}
    prev_cam = make_camera(W, H, look_from=(columns * z * cw / (W - 1), 0.0, 0.0))
    return guides, prev_cam


def cornell_at(dx, W=64, H=64):
    """tests/scenes.py's cornell box with the camera moved to look_from.x = 278 - dx (look_at unchanged)."""
    import scenes
    from sightpy import vec3

    sc = scenes.cornell(W, H)
    sc.add_Camera(screen_width=W, screen_height=H, look_from=vec3(278 - dx, 278, 800), look_at=vec3(278, 278, 0),
                  focal_distance=1.0, field_of_view=40)
    return sc


FIXTURE_DX = (18, 12, 6)  # the three earlier frames of tests/golden/temporal_cornell_64x64.npz; the fourth is at 0


@functools.lru_cache(maxsize=1)
def fixture_frames():
    """The four frames of the quality fixture, oldest first: [(A, B, guides, camera_dict)].  The first three are
    temporal_cornell_64x64's, the fourth is denoise_var_cornell_64x64's halves at the fixture camera.  Guides from
    the oracle (tests/denoise_ref.py aovs).  Computed once and shared; treat as read-only."""
    import denoise_ref as DR
    from conftest import golden

    g, g1 = golden("temporal_cornell_64x64"), golden("denoise_var_cornell_64x64")
    frames = []
    for k, dx in enumerate(FIXTURE_DX + (0,)):
        sc = cornell_at(dx)
        A, B = (g["half_a_%d" % k], g["half_b_%d" % k]) if dx else (g1["half_a"], g1["half_b"])
        frames.append((A, B, DR.aovs(sc), camera_dict(sc.camera)))
    return frames


def accumulate_sequence(frames, W, H, run, **kw):
    """`run` (accumulate's signature) over `frames` in order, each call's history the one before's: the last
    call's result."""
    hist, cam, out = None, None, None
    for A, B, guides, c in frames:
        out = run(A, B, guides, W, H, history=hist, prev_cam=cam, **kw)
        hist, cam = next_history(out, guides), c
    return out


def fixture_error_ratios(run, filt, levels=(0, 3)):
    """E / E(the last frame's unfiltered mean) on the quality fixture, E = denoise_ref.tonemapped_error against the
    64-sample `ref` of denoise_cornell_64x64: ({levels: accumulated by `run`, then filtered by `filt`},
    {levels: the last frame alone, filtered by `filt`}).  filt(A, B, ka, kb, guides, W, H, variance=, demodulate=,
    levels=) -> (c', ...)."""
    import denoise_ref as DR
    import denoise_var_ref as VR
    from conftest import golden

    frames = fixture_frames()
    ref = golden("denoise_cornell_64x64")["ref"]
    A, B, guides, _ = frames[-1]
    out = accumulate_sequence(frames, 64, 64, run, demodulate=True)
    e0 = DR.tonemapped_error(VR.mean_of_halves(A, B, 2, 2), ref)
    f = lambda a, b, l: DR.tonemapped_error(filt(a, b, 2, 2, guides, 64, 64, variance=True, demodulate=True, levels=l)[0],
                                            ref) / e0
    return {l: f(out["a"], out["b"], l) for l in levels}, {l: f(A, B, l) for l in levels}


# ---- the checks both suites run; `run` has accumulate's signature (without `info`) and result -------------------
def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_against_restatement(run, W, H, demodulate, with_history):
    """`run` on random_sequence(W, H) against accumulate, and the pixels the definition copies through."""
    from denoise_ref import close

    s = random_sequence(W, H, 10 * W + H)
    A, B, guides = s["A"], s["B"], s["guides"]
    kw = dict(history=s["history"], prev_cam=s["prev_cam"]) if with_history else {}
    info = {}
    ref = accumulate(A, B, guides, W, H, demodulate=demodulate, info=info, **kw)
    got = run(A, B, guides, W, H, demodulate=demodulate, **kw)
    for k in OUTPUTS:
        close(got[k], ref[k])
    bg = guides["hit_id"] < 0
    bad = np.zeros(W * H, dtype=bool)
    if s["inf"] is not None:
        bad[[s["inf"], s["nan"]]] = True
        assert bg.any()
    ok = ~bg & ~bad
    has = info["has"]
    # background, non-finite and disoccluded pixels (all of them on a first frame): A and B themselves
    for keep in (bg, bad, ok & ~has):
        assert same_bits(got["a"][:, keep], A[:, keep]) and same_bits(got["b"][:, keep], B[:, keep])
    assert not got["len"][bg | bad].any() and (got["len"][ok & ~has] == 1.0).all()
    for keep in (bg, bad):
        assert same_bits(got["hist_a"][:, keep], A[:, keep]) and same_bits(got["hist_b"][:, keep], B[:, keep])
    if not with_history:
        assert not has.any()
        if not demodulate:
            assert same_bits(got["hist_a"], A) and same_bits(got["hist_b"], B)
    elif W * H > 1:
        # the generator's scene gives every kind of pixel: history found, and refused
        assert has.any() and (ok & ~has).any() and (got["len"][has] > 1.0).all()
        assert np.abs(got["a"][:, has] - A[:, has]).max() > 1e-3
    return got, ref, info


def check_exact_shift(run, columns):
    """A wall facing the camera, the previous camera `columns` (+1 or -1) pixel columns along `right`: the output is
    the history of column c - columns blended with the current colour at alpha = 1/2 (hist_len 1), within 1e-9."""
    W, H = 9, 4
    n = W * H
    guides, prev_cam = shifted_plane(W, H, columns)
    rng = np.random.default_rng(11)
    A, B = rng.random((3, n)), rng.random((3, n))
    hist = {"a": rng.random((3, n)), "b": rng.random((3, n)), "len": np.ones(n), "hit_id": guides["hit_id"],
            "position": guides["position"], "normal": guides["normal"]}
    got = run(A, B, guides, W, H, history=hist, prev_cam=prev_cam)
    src = np.arange(W) - columns
    cols = (src >= 0) & (src < W)
    for k, cur in (("a", A), ("b", B)):
        h = hist[k].reshape(3, H, W)[:, :, src[cols]]
        c = cur.reshape(3, H, W)[:, :, cols]
        for name in (k, "hist_" + k):
            dev = np.abs(got[name].reshape(3, H, W)[:, :, cols] - (h + 0.5 * (c - h))).max()
            print("exact shift by", columns, name, "largest deviation", dev)
            assert dev <= 1e-9
    assert (got["len"].reshape(H, W)[:, cols] == 2.0).all()
    # the column that left the previous image has no history
    assert same_bits(got["a"].reshape(3, H, W)[:, :, ~cols], A.reshape(3, H, W)[:, :, ~cols])
    assert (got["len"].reshape(H, W)[:, ~cols] == 1.0).all()


def check_static_mean(run):
    """An unchanged camera over the cornell guides: the fixture's half-frames, then four frames of random colours.
    After the five calls len is 5 on every ok pixel and out_a is the arithmetic mean of the five A's within 1e-8
    relative (denominator floor 1e-3); the residue is the projection's rounding (about 1e-13 pixel) letting in
    a neighbour's colour."""
    import denoise_ref as DR
    from conftest import golden

    g = golden("denoise_var_cornell_64x64")
    W = H = 64
    sc = cornell_at(0, W, H)
    guides, cam = DR.aovs(sc), camera_dict(sc.camera)
    rng = np.random.default_rng(5)
    frames = [(g["half_a"], g["half_b"], guides, cam)] + \
             [(rng.random((3, W * H)), rng.random((3, W * H)), guides, cam) for _ in range(4)]
    out = accumulate_sequence(frames, W, H, run)
    ok = (guides["normal"] != 0.0).any(axis=0) & np.isfinite(g["half_a"]).all(axis=0) & np.isfinite(g["half_b"]).all(axis=0)
    assert ok.sum() > 0.8 * W * H and (out["len"][ok] == 5.0).all()
    worst = 0.0
    for k, i in (("a", 0), ("b", 1)):
        mean = sum(f[i] for f in frames) / 5.0
        worst = max(worst, float((np.abs(out[k] - mean) / np.maximum(np.abs(mean), 1e-3))[:, ok].max()))
    print("static camera, 5 frames: largest relative deviation from the arithmetic mean", worst)
    assert worst <= 1e-8


def check_max_history(run):
    """len never exceeds max_history, and the blend weight stops at 1 / max_history."""
    W, H = 9, 4
    n = W * H
    guides, _ = shifted_plane(W, H, 1)
    cam = make_camera(W, H)
    rng = np.random.default_rng(2)
    frames = [(rng.random((3, n)), rng.random((3, n)), guides, cam) for _ in range(5)]
    hist, out = None, None
    for i, (A, B, _, _) in enumerate(frames):
        prev = hist
        out = run(A, B, guides, W, H, history=hist, prev_cam=cam if hist else None, max_history=3)
        assert (out["len"] == min(i + 1, 3)).all()
        hist = next_history(out, guides)
    # the fifth call: alpha = 1/3 on the fourth call's history
    want = prev["a"] + (frames[-1][0] - prev["a"]) * (1.0 / 3.0)
    assert np.abs(out["a"] - want).max() <= 1e-9
