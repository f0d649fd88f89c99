"""The two paths of the device generator of numpy's stream (rt_mt_kernel.h k_mt_gen): runs of whole
blocks go four 624-word blocks at a time (a super-iteration, entered at ring slot 0 or 4), everything
else -- a segment's first and last blocks, plane crossings, masked bands, the chain and dump windows
-- a block at a time.  The sizes below are the smallest that cross each boundary of that structure.
Oracle: numpy itself (np.random.RandomState), bit for bit: the doubles with array_equal, the final
state with get_state(); through the render path (plane masks, a shard's rows, pipelined frames: the
library hands out no jitter), the frame rendered from numpy's own draws (the same jitter gives the same
image: the framebuffer sums are order-independent) and numpy's state after it."""
import ctypes

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SEG = 1 << 18     # doubles per tabulated segment
BLOCK = 312       # doubles per 624-word block


def _numpy(st, n_out, n_skip=0):
    rs = np.random.RandomState()
    rs.set_state(st)
    want = rs.random_sample(n_out)
    rs.random_sample(n_skip)
    return want, rs.get_state()


def _device(st, n_out, n_skip=0):
    from sightpy import _backend as B

    np.random.set_state(st)
    got = np.empty(n_out)
    B.numpy_uniforms(n_out, n_skip, out=got)
    return got, np.random.get_state()


def _same_state(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1])


def _residue():
    from sightpy import _backend as B, _native as N

    lib, ctx = B.context()
    nz = ctypes.c_int64(-1)
    N.check(lib, lib.srt_debug_mt_residue(ctx, ctypes.byref(nz)))
    return nz.value


@pytest.mark.parametrize("pos", [0, 1, 2, 623, 624])
def test_start_positions_three_segments(pos):
    """3 x 2^18 + 7 doubles (three segments, the last partial) from key position `pos`: an odd position
    puts every pair across two words of different parity, the first pair of a block across two blocks."""
    key = np.random.RandomState(100 + pos).get_state()[1]
    st = ("MT19937", key, pos, 0, 0.0)
    want, end = _numpy(st, 3 * SEG + 7)
    got, after = _device(st, 3 * SEG + 7)
    assert np.array_equal(got, want)
    assert _same_state(after, end)


@pytest.mark.parametrize("pos", [10, 11])
@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5, 9])
def test_whole_block_run_lengths(pos, blocks):
    """A partial first block, then 1, 2, 3, 4, 5 and 9 whole blocks -- every remainder of the
    super-iteration of 4 (no run, one super-iteration, one and a block, two and a block) -- from an even
    and an odd key position, ending on a block edge and 5 doubles past it.  The final window is dumped
    by the generator, inside or right after the run."""
    key = np.random.RandomState(7).get_state()[1]
    st = ("MT19937", key, pos, 0, 0.0)
    first = BLOCK - (pos + 1) // 2  # pairs whose second word block 0 holds
    for tail in (0, 5):
        n = first + BLOCK * blocks + tail
        want, end = _numpy(st, n)
        got, after = _device(st, n)
        assert np.array_equal(got, want), (blocks, tail)
        assert _same_state(after, end), (blocks, tail)


def test_chained_calls_start_from_the_dumped_state_and_rezero_the_windows():
    """Two consecutive calls of three segments, the second from the state the first dumped: its jump
    parts XOR into the segment windows, which the first call's generators must have left zero."""
    st = np.random.RandomState(21).get_state()
    n = 2 * SEG + 1001
    want1, mid = _numpy(st, n, 3)
    want2, end = _numpy(mid, n, 0)
    got1, after1 = _device(st, n, 3)
    assert _residue() == 0
    assert _same_state(after1, mid)
    got2, after2 = _device(after1, n, 0)
    assert _residue() == 0
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
    assert _same_state(after2, end)


def _frame_pair(sc, spp, rows=None):
    """(frame from the device stream, numpy state after it), (frame from numpy's own draws, state)."""
    from sightpy import _backend as B

    W, H = int(sc.camera.screen_width), int(sc.camera.screen_height)
    np.random.seed(9)
    a = B.render_scene(sc, spp, seed=1, mt=True, rows=rows)
    sa = np.random.get_state()
    np.random.seed(9)
    jit = sc.camera.draw_jitter(spp)
    np.random.rand(4 * W * H)  # the reference's sizing draw
    sb = np.random.get_state()
    if rows is not None:
        jit = np.ascontiguousarray(jit.reshape(spp, 4, H, W)[:, :, rows].reshape(spp, 4, -1))
    b = B.render_scene(sc, spp, jitter=jit, seed=1, rows=rows)
    return (a, sa), (b, sb)


# plane sizes (doubles per jitter plane = pixels): the issue's five -- a plane begins and ends inside a
# block, on a block edge, and around a segment edge -- and 3072 (64 x 48): plane edges every 9.8 blocks,
# all but a few of them in mid-segment
PLANES = [(311, 1), (24, 13), (313, 1), (511, 513), (17497, 15), (64, 48)]


@pytest.mark.parametrize("lens", [0.0, 0.05], ids=["mask0011", "mask1111"])
@pytest.mark.parametrize("wh", PLANES, ids=["311", "312", "313", "2^18-1", "2^18+311", "3072"])
def test_plane_masks_tabulated_segments(wh, lens):
    """Frames whose jitter planes hold 311, 312, 313, 2^18 - 1, 2^18 + 311 and 3072 doubles, pinhole
    (mask 0b0011: planes 2 and 3 of every sample are not read) and thin lens (0b1111), generated in the
    tabulated segments (option mt_short = 0) and in band mode (the default).

    What each reaches in k_mt_gen.  Tabulated segments apply the plane mask only to planes of at least
    1024 doubles (smaller ones are all stored: a block would span more than two planes), so 311, 312
    and 313 run there unmasked, as runs of whole blocks through every plane edge.  2^18 - 1, 2^18 + 311
    and 3072 run with the mask: with the pinhole, blocks change stored -> skipped -> stored and a run of
    whole blocks ends at the plane's edge (kstop = min(kend, kb)), for 3072 every 9.8 blocks in
    mid-segment, for the two large ones around a segment's edge; with the thin lens the runs end at
    every plane edge and go on in the next plane.  Band mode makes a segment of every stored plane (no
    mask in the kernel): the planes' sizes are the segments' lengths there, so 311, 312 and 313 are
    segments of one partial block, exactly one block, and one block and a pair.

    The library hands out no jitter, so the doubles are compared through the frame they give: a wrong
    double in a plane the camera reads changes the fp64 image; the planes the pinhole skips are not
    checked, and need not be right (they are not generated to be read)."""
    from sightpy import _backend as B, _native as N

    assert wh[0] * wh[1] in (311, 312, 313, SEG - 1, SEG + 311, 3072)
    lib, ctx = B.context()
    sc = scenes.example1(wh[0], wh[1], 2)
    sc.camera.lens_radius = lens
    for short in (0, 65536):
        N.check(lib, lib.srt_set_option(ctx, b"mt_short", short))
        try:
            (a, sa), (b, sb) = _frame_pair(sc, 2)
        finally:
            N.check(lib, lib.srt_set_option(ctx, b"mt_short", 65536))
        assert _residue() == 0
        assert np.array_equal(a.rgb, b.rgb) and np.array_equal(a.srgb8, b.srgb8), short
        assert _same_state(sa, sb), short


@pytest.mark.parametrize("bands", [1, 0], ids=["compact", "frame-layout"])
@pytest.mark.parametrize("lens", [0.0, 0.05], ids=["mask0011", "mask1111"])
@pytest.mark.parametrize("ranks,rank", [(8, 3), (2, 1)])
@pytest.mark.parametrize("band", [1, 2])
def test_band_mode_rows_of_one_rank(ranks, rank, band, lens, bands):
    """The rows of rank 3 of 8 of a 64 x 48 frame, in bands of 1 and 2 rows, in both layouts of a
    shard's jitter: equal to the same rows cut from numpy's full draw, and numpy's state moves past the
    whole frame's draws.
      compact (option mt_bands = 1, the default): band mode, only the rows' runs are generated, into the
        shard's own layout.  The host merges runs into masked segments only when the gaps are no longer
        than the runs, which the rows of one rank of 8 never are; rank 1 of 2 is the pattern it merges,
        so that case is the one with the merged-band mask on.
      frame layout (mt_bands = 0): the whole frame's stream in the tabulated segments, in the frame's
        layout, with the plane mask: planes of 3072 doubles, so a run of whole blocks ends at a plane
        edge every 9.8 blocks.
    No host path produces a masked band in the frame's layout: band mode always stores compact
    (mt_launch_bands), so that combination of the kernel's arguments is not reachable through the
    library."""
    from sightpy import _backend as B, _native as N

    lib, ctx = B.context()
    sc = scenes.example1(64, 48, 2)
    sc.camera.lens_radius = lens
    rows = [r for r in range(48) if (r // band) % ranks == rank]
    N.check(lib, lib.srt_set_option(ctx, b"mt_bands", bands))
    try:
        (a, sa), (b, sb) = _frame_pair(sc, 2, rows=rows)
    finally:
        N.check(lib, lib.srt_set_option(ctx, b"mt_bands", 1))
    assert _residue() == 0
    assert np.array_equal(a.rgb, b.rgb) and np.array_equal(a.srgb8, b.srgb8)
    assert _same_state(sa, sb)


def test_pipelined_frames_equal_synchronous_frames():
    """8 pipelined ex1 frames at 160 x 120, 6 spp (k_mt_gen<256> beside the trace kernel, the frame-end
    jump and y_next handing the key on) equal the same frames rendered one at a time."""
    from sightpy import _backend as B, _native as N

    lib, ctx = B.context()
    sc = scenes.example1(160, 120, 5)
    nf, spp, npix = 8, 6, 160 * 120
    np.random.seed(31)
    sync = [B.render_scene(sc, spp, seed=5, mt=True) for _ in range(nf)]
    s_sync = np.random.get_state()
    np.random.seed(31)
    mt = N.MtState.from_numpy()
    B.upload(sc)
    cd = B.camera_desc(sc.camera)
    bufs = [(B.device_buffer("paths_rgb%d" % k, 3 * npix * 8), B.device_buffer("paths_u8%d" % k, 3 * npix))
            for k in range(nf)]
    a = N.RenderArgs()
    a.spp, a.sample_base, a.n_rows, a.batch_spp = spp, 0, 120, 0
    a.jitter, a.seed, a.out_hit_id, a.rows = None, 5, None, None
    a.mt = ctypes.pointer(mt)
    a.flags = N.RENDER_ASYNC
    for k in range(nf):
        a.out_rgb, a.out_srgb8 = bufs[k]
        N.check(lib, lib.srt_render(ctx, ctypes.byref(cd), ctypes.byref(a), None))
    N.check(lib, lib.srt_render_finish(ctx, None))
    mt.to_numpy()
    assert _residue() == 0
    assert _same_state(np.random.get_state(), s_sync)
    for k in range(nf):
        rgb = np.empty((3, npix))
        N.check(lib, lib.srt_memcpy(ctx, N.ptr(rgb), bufs[k][0], rgb.nbytes))
        assert np.array_equal(rgb, sync[k].rgb), k
