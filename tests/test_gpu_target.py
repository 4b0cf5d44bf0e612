"""-m gpu: the device-resident framebuffer (srz_target_*: srz.Target) against the oracle, bit for bit.

The target is the one place where the library keeps state between calls: z and colour planes that stay in HBM, and a clear(Color|Depth)
that is only a flag until the next draw (which then runs with SRZ_FUSED_CLEAR), read or partial clear.  Every comparison here is of
words (support.same / uint32 views) against orc.draw of the same frames over the same incoming planes, and against orc.resolve8 for the
bytes; there is no tolerance in this module.  Frames carry flags = 0: whether a draw clears is the target's own state, never the
frame's.  Conditions stated "from the oracle alone" are asserted inside the case builders below, which need no device."""
import functools

import numpy as np
import pytest

import scenes
from srz import abi
from support import (HOSTILE_TEX, Z_CLEAR, assert_clear, bits, ccw, copy_planes, ctx, frame, oracle_draws,  # noqa: F401  (ctx: the fixture)
                     overhang_pair, place, register_hostile_textures, same, scene_pair, sceneset_update, soup, unshared_mesh)

pytestmark = pytest.mark.gpu

IDENT = np.eye(4, dtype=np.float32).reshape(16)
NRM_UP = (0.0, 0.0, -1.0)


def draw_frame(ctx, t, f, **kw):
    """frame f through a one-frame set of its own into target t (the set is gone afterwards) -> the draw's counters or None"""
    fs = ctx.frameset([f])
    try:
        return t.draw(fs, **kw)
    finally:
        fs.close()


def canary(h, w):
    return np.full((h, w), np.float32(-12345.5), np.float32)


# ------------------------------------------------------------------------------------------------ a. fresh and failed
def small_frame(w=64, h=64, n=1, shift=0.0):
    t = np.concatenate([ccw((6 + shift, 5), (40.5 + shift, 9), (11 + shift, 44.25), z=30.0 + k, nrm=(0.3, -0.2, -1.0)) for k in range(n)])
    return frame(t, w=w, h=h, flags=0)


def refusals(ctx, t):
    """[(what, call, code, text)]: the draws srz_target_draw refuses for a 64 x 64 target t; the sets are made here and closed by the
    caller (the last entry of each tuple)"""
    import srz
    other_size = ctx.frameset([small_frame(32, 32)])
    two_frames = ctx.frameset([small_frame(), small_frame(shift=3.0)])
    ctx.set_shard(1, 3)
    try:
        sharded = ctx.frameset([small_frame()])
    finally:
        ctx.set_shard(0, 1)
    ok_set = ctx.frameset([small_frame()])
    assert isinstance(t, srz.Target) and (t.width, t.height) == (64, 64)
    invalid = "needs an unsharded 1-frame set of the target's size"
    return [("another size", lambda: t.draw(other_size), abi.SRZ_E_INVALID, invalid, other_size),
            ("two frames", lambda: t.draw(two_frames), abi.SRZ_E_INVALID, invalid, two_frames),
            ("a sharded context's set", lambda: t.draw(sharded), abi.SRZ_E_INVALID, invalid, sharded),
            ("primitive 7", lambda: t.draw(ok_set, primitive=7), abi.SRZ_E_PRIMITIVE, "Primitive Type is not supported!", ok_set)]


def check_refusals(ctx, t):
    import srz
    cases = refusals(ctx, t)
    try:
        for what, call, code, text, _ in cases:
            with pytest.raises(srz.SrzError) as e:
                call()
            assert e.value.code == code and text in str(e.value), (what, e.value.code, str(e.value))
    finally:
        for c in cases:
            c[-1].close()


def test_fresh_target_holds_the_clear_values(ctx):
    """srz_target_create never writes the planes: what a read returns straight after it is the deferred clear materialised, not
    whatever the allocation held.  Both reads, on targets of their own (the first read clears the flag)."""
    t = ctx.target(64, 64)
    assert_clear(t.read(), "create, read")
    assert_clear(t.read(), "create, read, read")
    assert not t.read_bgr8().any()
    t.close()
    t = ctx.target(33, 31)  # (first call on a fresh target: the resolve, which must materialise the clear as well)
    assert not t.read_bgr8().any(), "create, read_bgr8"
    assert_clear(t.read(), "create, read_bgr8, read")
    t.close()


def test_refused_draw_leaves_a_fresh_target_cleared(ctx):
    """a draw that is refused must leave the pending clear in place: each refusal returns its documented code and text, and the read
    that follows gives the clear values"""
    t = ctx.target(64, 64)
    check_refusals(ctx, t)
    assert_clear(t.read(), "create, refused draws, read")
    assert not t.read_bgr8().any()
    t.close()


def test_refused_draw_leaves_the_planes_of_an_earlier_draw(ctx, orc):
    t = ctx.target(64, 64)
    a = small_frame(n=3)
    (ref,), _ = oracle_draws(orc, [a])
    assert np.isfinite(ref[0]).sum() > 300
    draw_frame(ctx, t, a)
    same(t.read(), ref, "draw A")
    check_refusals(ctx, t)
    same(t.read(), ref, "draw A, refused draws")
    assert np.array_equal(t.read_bgr8(), orc.resolve8(ref))
    t.close()


# ------------------------------------------------------------------------------------------------ b. sizes
# size -> the resolve kernel launch_resolve8 picks for a target of it: k_resolve8 (four pixels a thread, a plane as one flat run)
# when rows * W is a multiple of 4, else k_resolve8_px
SIZES = {(1, 1): "px", (33, 31): "px", (101, 67): "px", (6, 2): "quad", (250, 130): "quad", (64, 64): "quad"}


@pytest.mark.parametrize("w,h", list(SIZES))
def test_sizes_planes_bytes_and_partial_reads(ctx, orc, w, h):
    """the two triangles of test_odd_sizes into a target of each size: planes = the oracle's, read_bgr8 = orc.resolve8 of them (the
    resolve on the target's own buffers: a W * H * 3 + 16 byte image, frame stride 4 planes).  Which kernel resolved follows from the
    size alone and is asserted, so that both are known to have run: (6, 2) and (250, 130) take the quad kernel with W % 4 != 0, where
    its flat run crosses row ends.  A read of z alone, and of c1 alone, fills that plane and nothing next to it: the planes are
    slices of one canary-filled block, the skipped ones are passed as NULL."""
    assert ("quad" if (w * h) % 4 == 0 else "px") == SIZES[(w, h)]
    assert (w % 4 != 0) == ((w, h) != (64, 64))
    f = frame(overhang_pair(w, h), w=w, h=h, flags=0)
    (ref,), (rst,) = oracle_draws(orc, [f])
    assert rst["visible"] >= 1
    t = ctx.target(w, h)
    draw_frame(ctx, t, f)
    same(t.read(), ref, f"{w}x{h}")
    got8 = t.read_bgr8()
    want8 = orc.resolve8(ref)
    assert got8.shape == want8.shape == (h, w, 3)
    assert np.array_equal(got8, want8), f"{w}x{h}: {int((got8 != want8).sum())} bytes differ"
    same(t.read(), ref, f"{w}x{h} after the resolve")
    for only in (0, 2):
        block = np.stack([canary(h, w) for _ in range(6)])  # planes 1..4 are handed out, 0 and 5 guard the ends
        out = t.read(tuple(block[1 + p] if p == only else False for p in range(4)))
        assert [o is not None for o in out] == [p == only for p in range(4)]
        assert np.array_equal(bits(block[1 + only]), bits(ref[only])), f"{w}x{h}: plane {only} read alone"
        for k in range(6):
            if k != 1 + only:
                assert np.array_equal(bits(block[k]), bits(canary(h, w))), f"{w}x{h}: reading plane {only} alone wrote into slice {k}"
    t.close()


# ------------------------------------------------------------------------------------------------ c. accumulation on the device
C_W = C_H = 64
TIE_Z = 64.0  # flat, a power of two: with areas that are powers of two and half-pixel vertices both classes interpolate it exactly


def tie_triangles():
    """(A's V triangle, B's S triangle over it; A's S triangle, B's V triangle over it), all at z = TIE_Z.  A triangle whose box is
    narrower than 8 columns has scalar-tail (S) columns only and passes z <= stored: drawn later it takes a tied pixel.  The first
    8-wide columns of a wide box are V columns and pass z < stored only: drawn later it loses a tied pixel."""
    a_v = ccw((4.5, 4.5), (36.5, 4.5), (4.5, 36.5), z=TIE_Z, nrm=NRM_UP)
    b_s = ccw((8.5, 8.5), (12.5, 8.5), (8.5, 12.5), z=TIE_Z, nrm=(1.0, 0.0, 0.0))
    a_s = ccw((32.5, 32.5), (36.5, 32.5), (32.5, 36.5), z=TIE_Z, nrm=(0.0, 1.0, 0.0))
    b_v = ccw((28.5, 28.5), (60.5, 28.5), (28.5, 60.5), z=TIE_Z, nrm=(0.6, 0.0, -0.8))
    return a_v, b_s, a_s, b_v


def s_class_of(orc, f):
    """per pixel: frame f alone on fresh planes leaves a scalar-tail fragment there (the oracle's class probe)"""
    try:
        orc.debug_s(2)
        rc, cls, _ = orc.draw(f, want_stats=False)
    finally:
        orc.debug_s(0)
    assert rc == 0
    return cls[1] == -1.0


@functools.lru_cache(maxsize=None)
def accumulation_case():
    """-> (A, B, planes after A, after A B, after A B A; counters of the three draws).  From the oracle alone: the ties are ties, of
    the classes the docstring of tie_triangles names, visible in the composite and decided as those classes decide them; B changes
    pixels A owned and loses others; A over A B changes nothing."""
    from oracle import oracle as orc
    a_v, b_s, a_s, b_v = tie_triangles()
    zs = np.float32([20, 35, 50, 64, 80, 95])
    A = frame(np.concatenate([soup(4, 30, C_W, C_H, zs), a_v, a_s]), w=C_W, h=C_H, flags=0)
    B = frame(np.concatenate([b_s, soup(7, 30, C_W, C_H, zs), b_v]), w=C_W, h=C_H, flags=0)
    (pa, pab, paba), stats = oracle_draws(orc, [A, B, A])
    same(paba, pab, "the oracle: A over A B")  # idempotent in the oracle: the device must be too
    alone = {}
    for name, t in (("a_v", a_v), ("b_s", b_s), ("a_s", a_s), ("b_v", b_v)):
        f1 = frame(t, w=C_W, h=C_H, flags=0)
        rc, p, _ = orc.draw(f1)
        assert rc == 0
        alone[name] = (p, s_class_of(orc, f1))
    for first, second, second_wins in (("a_v", "b_s", True), ("a_s", "b_v", False)):
        (p1, s1), (p2, s2) = alone[first], alone[second]
        cov = np.isfinite(p1[0]) & np.isfinite(p2[0])
        tie = cov & (bits(p1[0]) == bits(p2[0])) & (s1 != s2) & (s2 == second_wins)  # an S triangle second wins, a V one loses
        assert tie.sum() >= 4, (first, second, int(cov.sum()), int(tie.sum()))
        # ... and the composite shows it: A left the first triangle there, and after B the pixel is the winner's
        shown = tie & np.logical_and.reduce([bits(pa[k]) == bits(p1[k]) for k in range(4)])
        win = p2 if second_wins else p1
        decided = shown & np.logical_and.reduce([bits(pab[k]) == bits(win[k]) for k in range(4)])
        assert decided.sum() >= 4, (first, second, int(shown.sum()), int(decided.sum()))
        assert any((bits(p1[k]) != bits(p2[k]))[decided].all() for k in (1, 2, 3))  # (the two colours differ: the winner shows)
    owned_a = np.isfinite(pa[0])
    diff = np.logical_or.reduce([bits(pa[k]) != bits(pab[k]) for k in range(4)])
    rc, b_alone, _ = orc.draw(B)
    assert rc == 0
    lost = owned_a & np.isfinite(b_alone[0]) & ~diff
    assert (owned_a & diff).sum() >= 50 and lost.sum() >= 50 and (~owned_a & diff).sum() >= 50, \
        (int((owned_a & diff).sum()), int(lost.sum()), int((~owned_a & diff).sum()))
    return A, B, pa, pab, paba, stats


@pytest.mark.parametrize("want_stats", [False, True])
def test_draws_accumulate_on_the_device(ctx, orc, want_stats):
    """draw A onto a pending clear (fused), then B and A again with flags = 0 onto the planes the earlier draws left in HBM: after
    each draw the target equals the oracle's sequence.  With stats every draw first copies the target into a scratch buffer and runs
    the counting kernels there: the counters equal the oracle's for that draw over those incoming planes, and the planes are the
    same as without (the copy leaves the target alone, the second pass agrees with the first)."""
    A, B, pa, pab, paba, rstats = accumulation_case()
    t = ctx.target(C_W, C_H)
    for k, (f, ref) in enumerate(((A, pa), (B, pab), (A, paba))):
        st = draw_frame(ctx, t, f, want_stats=want_stats)
        if want_stats:
            assert st == rstats[k], (k, st, rstats[k])
        else:
            assert st is None
        same(t.read(), ref, f"draw {k} of A B A, stats {want_stats}")
    assert np.array_equal(t.read_bgr8(), orc.resolve8(pab))
    t.close()


def test_draws_accumulate_without_a_read_in_between(ctx, orc):
    """the same sequence back to back, one read at the end (the reads of the test above synchronise after every draw)"""
    A, B, pa, pab, paba, _ = accumulation_case()
    t = ctx.target(C_W, C_H)
    sets = [ctx.frameset([A]), ctx.frameset([B])]
    for k in (0, 1, 0):
        t.draw(sets[k])
    same(t.read(), paba, "A B A back to back")
    for s in sets:
        s.close()
    t.close()


# ------------------------------------------------------------------------------------------------ d. clears
def test_clears(ctx, orc):
    """every path of srz_target_clear: a depth-only and a colour-only clear after a draw (the planes the next draw meets are exactly
    those); clear(1, 1) followed by a partial clear, which materialises the pending one first; followed by clear(0, 0), which must
    not drop it; twice; and clear(0, 0) on its own"""
    A, B, pa, _, _, _ = accumulation_case()
    w, h = C_W, C_H
    inf, zero = np.full((h, w), np.inf, np.float32), np.zeros((h, w), np.float32)
    (b_fresh,), _ = oracle_draws(orc, [B])
    sa, sb = ctx.frameset([A]), ctx.frameset([B])
    t = ctx.target(w, h)
    for color, depth in ((0, 1), (1, 0)):
        t.clear(1, 1)
        t.draw(sa)
        t.clear(color, depth)
        start = (inf if depth else pa[0],) + tuple(zero if color else p for p in pa[1:])
        same(t.read(), start, f"draw A, clear({color}, {depth})")
        (ref,), _ = oracle_draws(orc, [B], start)
        assert any((bits(ref[k]) != bits(b_fresh[k])).any() for k in range(4))  # (what A left does show in the result)
        t.draw(sb)
        same(t.read(), ref, f"draw A, clear({color}, {depth}), draw B")
    for second in ((0, 1), (1, 0), (0, 0), (1, 1)):
        t.clear(1, 1)
        t.clear(*second)
        t.draw(sb)
        same(t.read(), b_fresh, f"draw, clear(1, 1), clear{second}, draw B")
    for second in ((0, 1), (0, 0), (1, 1)):
        t.clear(1, 1)
        t.clear(*second)
        assert_clear(t.read(), f"draw, clear(1, 1), clear{second}, read")
        assert not t.read_bgr8().any()
        t.draw(sb)  # (planes to clear for the next round)
    same(t.read(), b_fresh, "clear values, draw B")
    t.clear(0, 0)
    same(t.read(), b_fresh, "draw B, clear(0, 0)")
    t.draw(sa)
    (ref,), _ = oracle_draws(orc, [A], b_fresh)
    same(t.read(), ref, "draw B, clear(0, 0), draw A")
    sa.close(), sb.close(), t.close()


# ------------------------------------------------------------------------------------------------ e. two kinds of set, one target
def small_mesh(seed, n=24, w=64, h=64, big=False):
    """n triangles in pixels as a mesh in unit coordinates (three vertices of its own per face), uv inside the texture"""
    t = soup(seed, n, w, h, np.float32([0.2, 0.4, 0.6, 0.8]), big)
    return unshared_mesh(t, w, h, seed)


def test_a_frameset_and_a_sceneset_alternate_into_one_target(ctx, orc):
    """a triangle frameset and a sceneset (device vertex stage, a TEXTURE draw among them) of one size drawn in turns into one
    target, a target of another size with sets of its own in between on the same context: each target equals its own oracle
    sequence — nothing of a set, or of the context, is carried from one target draw to the next"""
    register_hostile_textures(orc, ctx)
    lights = [((20.0, 10.0, 120.0), (900.0, 800.0, 700.0))]
    (v0, f0), (v1, f1) = small_mesh(11), small_mesh(12, n=9)
    draws = [(v0, f0, abi.SHADER_TEXTURE, HOSTILE_TEX, place(64.0, 64.0, 0.0, 0.0, sz=40.0, oz=20.0), IDENT),
             (v1, f1, abi.SHADER_NORMAL, -1, place(50.0, 40.0, 9.25, 14.5, sz=30.0, oz=25.0), IDENT)]
    sf, sf_as_frame = scene_pair(draws, 64, 64, (30.0, 20.0, 150.0), lights, 1.0, 0.0, flags=0, ctx=ctx, slots=[30, 31])
    tri = frame(soup(5, 40, 64, 64, np.float32([25, 35, 45, 55])), flags=0, shader=abi.SHADER_PHONG, lights=lights, eye=(30.0, 20.0, 150.0))
    other = [frame(overhang_pair(101, 67), w=101, h=67, flags=0), frame(soup(9, 30, 101, 67, np.float32([10, 61, 70])), w=101, h=67, flags=0)]
    order = [tri, sf_as_frame, tri, sf_as_frame]
    ref_main, st_main = oracle_draws(orc, order)
    ref_other, st_other = oracle_draws(orc, other + other)
    assert all(st["shaded"] > 0 for st in st_main + st_other) and st_main[1]["visible_textured"] > 100, (st_main, st_other)
    main, side = ctx.target(64, 64), ctx.target(101, 67)
    s_tri, s_scene = ctx.frameset([tri]), ctx.frameset([sf])
    s_other = [ctx.frameset([f]) for f in other]
    for k in range(4):
        main.draw(s_tri if k % 2 == 0 else s_scene)
        side.draw(s_other[k % 2])
        if k == 1:  # (once in the middle, once at the end)
            same(main.read(), ref_main[1], "main target after two draws")
            same(side.read(), ref_other[1], "side target after two draws")
    same(main.read(), ref_main[3], "main target")
    same(side.read(), ref_other[3], "side target")
    assert np.array_equal(main.read_bgr8(), orc.resolve8(ref_main[3])) and np.array_equal(side.read_bgr8(), orc.resolve8(ref_other[3]))
    for s in [s_tri, s_scene] + s_other:
        s.close()
    main.close(), side.close()


# ------------------------------------------------------------------------------------------------ f. updates in flight
F_SIZE, F_POSES, F_RING = 64, 9, 4  # (F_RING = STAGE_RING of csrc/srz_api.hip: the pinned staging buffers of a set's updates)


@functools.lru_cache(maxsize=None)
def poses_case():
    """-> (mesh, [(SceneFrame, Frame)] of the nine poses, the oracle's planes after each).  The poses step across the frame and come
    nearer (each overwrites a part of the one before), each with a normal matrix of its own (the NORMAL shader shows it).  From the
    oracle alone: the composite with pose k drawn from pose k + F_RING's matrices differs from the true one, for every k that has
    such a pose — a staging slot rewritten before its copy ran cannot pass."""
    from oracle import oracle as orc
    v, faces = small_mesh(21, n=40, big=True)
    pairs = []
    for k in range(F_POSES):
        nm = IDENT.copy()
        nm[0], nm[5], nm[15] = 1.0 + 0.25 * k, 1.0 - 0.0625 * k, 1.0 + k
        mvp = place(26.0, 24.0, 2.0 + 4.25 * k, 3.5 + (k % 3) * 13.0, sz=8.0, oz=60.0 - 5.0 * k)
        pairs.append(scene_pair([(v, faces, abi.SHADER_NORMAL, -1, mvp, nm)], F_SIZE, F_SIZE, (0.0, 0.0, 1.0), [], 1.0, 0.0, flags=0, slots=[33]))
    frames = [f for _, f in pairs]
    after, stats = oracle_draws(orc, frames)
    assert all(st["shaded"] > 100 for st in stats), stats  # (every pose writes pixels when its turn comes)
    for k in range(F_POSES - F_RING):
        wrong, _ = oracle_draws(orc, frames[:k] + [frames[k + F_RING]] + frames[k + 1:])
        n = int(np.logical_or.reduce([bits(wrong[-1][p]) != bits(after[-1][p]) for p in range(4)]).sum())
        assert n >= 20, (k, n)
    return (v, faces), pairs, after


def run_poses(ctx, busy):
    (v, faces), pairs, after = poses_case()
    ctx.mesh_upload(33, v, faces)
    fs = ctx.frameset([pairs[0][0]])
    t = ctx.target(F_SIZE, F_SIZE)
    if busy is not None:
        busy()
    for k, (sf, _) in enumerate(pairs):
        sceneset_update(ctx, fs, [sf], sync=False)
        t.draw(fs)
    same(t.read(), after[-1], "nine updates and draws, one read")
    fs.close(), t.close()


def test_nine_updates_in_flight(ctx):
    """srz_sceneset_update then srz_target_draw, nine times back to back on the context's stream, no clear, no read and no host
    synchronisation in between, more than twice the staging ring: the composite equals the oracle's nine draws"""
    run_poses(ctx, None)


def test_nine_updates_in_flight_behind_a_long_render(ctx):
    """the same nine pairs submitted while the context's stream is busy with a render of 24 frames of 1024 x 1024 (the benchmark's
    scene), so that the copies of the first updates have not run when the ring comes round.  This raises the chance of showing a
    staging slot reused too early; it does not guarantee it: how far the host gets ahead of the device is not under the test's
    control."""
    import torch
    frames = [scenes.config2(i) for i in range(3)]
    big = ctx.frameset([frames[i % 3] for i in range(24)])
    out = torch.empty(big.out_shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    run_poses(ctx, lambda: big.render(out.data_ptr(), big.out_bytes, abi.FUSED_CLEAR, None))  # (stream None: the context's own)
    ctx.sync()
    big.close()


# ------------------------------------------------------------------------------------------------ g. LINES and the empty set
def test_lines_and_empty_sets(ctx, orc):
    """PRIMITIVE_LINES draws filled triangles, as the oracle does.  A set that draws nothing: on a pending target the draw is the
    clear (a fused clear with no triangle must still write every pixel); on a target that holds a picture it changes nothing."""
    A, B, pa, pab, _, _ = accumulation_case()
    empty = ctx.frameset([frame(np.zeros(0, abi.TRI_DTYPE), w=C_W, h=C_H, flags=0)])
    no_batch = ctx.frameset([abi.Frame(C_W, C_H, (0, 0, 1), np.zeros((0, 2, 3), np.float32), [], 0)])
    sa, sb = ctx.frameset([A]), ctx.frameset([B])
    (lines_ref, lines_ab), _ = oracle_draws(orc, [A, B], primitive=abi.PRIMITIVE_LINES)
    same(lines_ab, pab, "the oracle: LINES = TRIANGLES")
    t = ctx.target(C_W, C_H)
    t.draw(sa, primitive=abi.PRIMITIVE_LINES)
    same(t.read(), lines_ref, "LINES onto a pending clear")
    t.draw(sb, primitive=abi.PRIMITIVE_LINES)
    same(t.read(), lines_ab, "LINES onto a picture")
    for k, e in enumerate((empty, no_batch)):
        st = t.draw(e, want_stats=bool(k))
        assert st is None or (st["n_tris"] == 0 and st["visible"] == 0), st
        same(t.read(), pab, "an empty set onto a picture")
        t.clear(1, 1)
        st = t.draw(e, want_stats=bool(k))
        assert st is None or (st["n_tris"] == 0 and st["visible"] == 0), st
        assert_clear(t.read(), "an empty set onto a pending clear")
        assert (bits(t.read()[0]) == Z_CLEAR).all()
        t.draw(sa), t.draw(sb)
        same(t.read(), pab, "A B after the empty draw")
    for s in (empty, no_batch, sa, sb):
        s.close()
    t.close()
