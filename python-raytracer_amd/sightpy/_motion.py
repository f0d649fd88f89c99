"""Per-collider motion between two consecutive frames, for srt_temporal_accumulate's `motion` table
(include/sightpy_rt.h): from two lowered collider tables (N.COLLIDER_DTYPE, the `colliders` of two uploads'
Lowered) one row of 12 doubles per collider, a 3x3 matrix R (row-major) and a vector t that map a point on the
collider in the current frame to the same surface point in the previous frame.  Vectorised numpy over the
records; the scene's Python objects are not consulted.

    a record whose bytes did not change:  exactly the identity row (a static object reprojects as without a table)
    tables of different lengths:          every row NaN (the list was reordered or edited: nothing can be matched)
    another type at the index, another size (a sphere's radius, a plane's w / h, a cuboid's width / height /
        length, a triangle's edge lengths beyond 1e-9 relative), or frames that give no rigid R
        (|R^T R - I| > 1e-9):             a NaN row, which leaves that collider's pixels without history
    SPHERE    R = I, t = c_prev - c_cur
    PLANE     F = [u_axis v_axis normal] as columns, R = F_prev F_cur^T, t = c_prev - R c_cur
    CUBOID    F = [ax_w ax_h ax_l] as columns, likewise
    TRIANGLE  E = [p2 - p1, p3 - p1, normal] as columns, R = E_prev E_cur^-1, t = p1_prev - R p1_cur
"""
import numpy as np

from . import _native as N

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
RIGID_TOL = 1e-9  # largest |R^T R - I| entry of a row that is kept, and the relative change of a triangle's edges


def _columns(p, *slices):
    """(n, 3, 3): the vectors p[:, s] of each record as the columns of a matrix."""
    return np.stack([p[:, s] for s in slices], axis=2)


def _put(out, sel, R, t_prev, t_cur):
    """Rows `sel` of `out` from R (n, 3, 3) and t = t_prev - R t_cur; NaN where R is not a rotation."""
    R = R[sel]
    rigid = np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).reshape(-1, 9).max(axis=1) <= RIGID_TOL
    rows = np.concatenate([R.reshape(-1, 9), t_prev[sel] - np.einsum("nij,nj->ni", R, t_cur[sel])], axis=1)
    rows[~rigid] = np.nan
    out[sel] = rows


def collider_motion(prev_table, cur_table):
    """(n, 12) float64, n = len(cur_table): the module comment's rows."""
    prev, cur = np.asarray(prev_table), np.asarray(cur_table)
    n = len(cur)
    out = np.full((n, 12), np.nan)
    if len(prev) != n or n == 0:
        return out
    pp, pc = prev["p"], cur["p"]
    typ = cur["type"]
    same_type = prev["type"] == typ
    with np.errstate(all="ignore"):
        m = same_type & (typ == N.SPHERE) & (pp[:, 3] == pc[:, 3])
        out[m, :9] = IDENTITY[:9]
        out[m, 9:] = pp[m, 0:3] - pc[m, 0:3]

        m = same_type & (typ == N.PLANE) & (pp[:, 12] == pc[:, 12]) & (pp[:, 13] == pc[:, 13])
        if m.any():
            frame = lambda p: _columns(p, slice(6, 9), slice(9, 12), slice(3, 6))
            _put(out, m, np.einsum("nik,njk->nij", frame(pp), frame(pc)), pp[:, 0:3], pc[:, 0:3])

        m = same_type & (typ == N.CUBOID) & (pp[:, 27:30] == pc[:, 27:30]).all(axis=1)
        if m.any():
            frame = lambda p: _columns(p, slice(18, 21), slice(21, 24), slice(24, 27))
            _put(out, m, np.einsum("nik,njk->nij", frame(pp), frame(pc)), pp[:, 0:3], pc[:, 0:3])

        m = same_type & (typ == N.TRIANGLE)
        if m.any():
            def edges(p):
                e = np.stack([p[:, 9:12] - p[:, 6:9], p[:, 12:15] - p[:, 6:9], p[:, 12:15] - p[:, 9:12]], axis=1)
                return np.sqrt((e * e).sum(axis=2))

            lp, lc = edges(pp), edges(pc)
            m &= (np.abs(lp - lc) <= RIGID_TOL * np.maximum(lp, lc)).all(axis=1)
        if m.any():
            frame = lambda p: np.stack([p[m, 9:12] - p[m, 6:9], p[m, 12:15] - p[m, 6:9], p[m, 3:6]], axis=2)
            Ep, Ec = frame(pp), frame(pc)
            ok = np.abs(np.linalg.det(Ec)) > 0.0  # (a degenerate triangle has no inverse: its row stays NaN)
            R = np.full((n, 3, 3), np.nan)
            R[np.flatnonzero(m)[ok]] = Ep[ok] @ np.linalg.inv(Ec[ok])
            _put(out, m, R, pp[:, 6:9], pc[:, 6:9])
    # an unchanged record: the identity, exactly
    same = (prev.view(np.uint8).reshape(n, -1) == cur.view(np.uint8).reshape(n, -1)).all(axis=1)
    out[same] = IDENTITY
    return out


def pose_motion(rows, prev_posed, cur_posed):
    """Overwrite, in `rows` (collider_motion's table of the two frames), the rows of the device-posed meshes of
    the current frame (`cur_posed`, `prev_posed`: the Lowered.posed lists of the two frames).  Such a mesh's records
    are its rest pose in both tables, so collider_motion calls it static; its motion is the pose pair's: a
    point x of the current frame was at R_prev R_cur^T (x - T_cur) + T_prev (R_cur is a rotation: its inverse
    is its transpose), the same row for every collider of the mesh -- the records are not looked at.  Equal
    poses give the identity row exactly.  A mesh without an entry of the same key and range in `prev_posed`
    (first posed in this frame, invalidated or moved in the list since) gets NaN rows, and so does a mesh whose
    vertex version ("vver", read with .get: TriangleMesh.set_vertices) differs between the two frames: its shape
    changed, no rigid row describes that, and it has no history."""
    prev = {p["key"]: p for p in prev_posed}
    for cur in cur_posed:
        sl = slice(cur["first"], cur["first"] + cur["count"])
        old = prev.get(cur["key"])
        if (old is None or (old["first"], old["count"]) != (cur["first"], cur["count"])
                or old.get("vver") != cur.get("vver")):
            rows[sl] = np.nan
        elif np.array_equal(old["pose"], cur["pose"]):
            rows[sl] = IDENTITY
        else:
            Rp, Rc = old["pose"][:9].reshape(3, 3), cur["pose"][:9].reshape(3, 3)
            R = Rp @ Rc.T
            rows[sl] = np.concatenate([R.reshape(-1), old["pose"][9:] - R @ cur["pose"][9:]])
    return rows


def count_rows(motion):
    """(moved, unknown) of a table: rows that are neither the identity nor NaN, and rows holding a NaN."""
    unknown = np.isnan(motion).any(axis=1)
    moved = ~unknown & (motion != IDENTITY).any(axis=1)
    return int(moved.sum()), int(unknown.sum())
