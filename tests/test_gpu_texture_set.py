"""-m gpu: texture sets (srz_frameset_texture_set / _texture_set_grad, k_tex_set, k_tex_set_grad): the caller's texture of each pixel
picked by its owner's batch.  The visibility buffer is the GPU's own render_visibility and uv the GPU's own interpolate of the
frames' uv, except where a test writes the planes by hand; the expected values are tests/texsetref.py's — a composition of
tests/texref.py per slot, pinned on the CPU by tests/test_texset_ref.py together with the properties of the cases used here.
Forward and guv: a NaN on one side must be a NaN on the other, every other word matches bit for bit.  gtex, per slot: exact in the
dyadic cases, else within texref.Grad.bound — gamma_n * sum |w g|, n the element's contributing adds: derived, not measured."""
import numpy as np
import pytest
import torch

import texref
import texsetref
from srz import abi
from support import SENTINEL, ccw, ctx, filled, frame, place, scene_pair, soup, stack, stream, unshared_mesh, visibility, words  # noqa: F401
from texref import CLAMP, WRAP
from walkkit import same

pytestmark = pytest.mark.gpu

F = abi.FUSED_CLEAR
ZS = texref.ZS
TEX_SIZES = ((1, 1), (5, 7), (33, 1), (64, 64))  # (tex_w, tex_h), mixed in one call
CHANNELS = (1, 3, 5, 64)  # (64: ATTR_CHUNK's tail is empty; 1, 3, 5: it is not)
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def split(t, k):
    return [(abi.SHADER_NORMAL, -1, np.ascontiguousarray(t[i::k])) for i in range(k)]


def interp_uv(fs, vis, frames):
    """the GPU's interpolate of the frames' own uv → the planes on the device [n, 2, rows, W] and as an array"""
    T = max(f.n_tris for f in frames)
    a = np.zeros((len(frames), T, 3, 2), np.float32)
    for i, f in enumerate(frames):
        a[i, :f.n_tris] = texref.frame_uv(f)
    out, a_dev = torch.zeros(fs.interpolate_shape(2), dtype=torch.float32, device="cuda"), dev(a)
    fs.interpolate(vis.data_ptr(), a_dev.data_ptr(), 2, len(frames), T, out.data_ptr(), fs.interpolate_bytes(2), F, stream())
    torch.cuda.synchronize()
    return out, out.cpu().numpy()


def make_texs(seed, C, n_frames, sizes=TEX_SIZES, n=None):
    """n textures (default: one per size), the sizes in turn, every other one per frame; texels normal values"""
    n = len(sizes) if n is None else n
    return [texref.make_tex(seed + s, *sizes[s % len(sizes)], C, frames=n_frames if s % 2 else None) for s in range(n)]


def map_dev(batch_slot):
    return torch.tensor([texsetref.NONE if s is None else s for s in batch_slot], dtype=torch.uint8, device="cuda")


def slot_tuples(texs, t_dev, modes, gtexs=None):
    return [(t_dev[s].data_ptr() if t_dev[s] is not None else None, gtexs[s].data_ptr() if gtexs and gtexs[s] is not None else None,
             t.shape[-2], t.shape[-3], t.shape[0] if t.ndim == 4 else 1, modes[s]) for s, t in enumerate(texs)]


def upload(texs, share=None):
    """one device tensor per texture — or, for a slot s of share {s: other slot}, the OTHER slot's tensor: one d_tex for both"""
    t_dev = [dev(t) for t in texs]
    for s, src in (share or {}).items():
        assert texs[s] is texs[src]
        t_dev[s] = t_dev[src]
    return t_dev


def fwd(fs, vis, uv, texs, modes, batch_slot, flags=F, fill=SENTINEL, share=None):
    """the forward pass into a buffer prefilled with the word `fill` → uint32 [n, C, rows, W]"""
    C, t_dev, m = texs[0].shape[-1], upload(texs, share), map_dev(batch_slot)
    out = filled(fs.interpolate_shape(C), fill)
    fs.texture_set(vis.data_ptr(), uv.data_ptr(), slot_tuples(texs, t_dev, modes), m.data_ptr(), len(batch_slot), C, out.data_ptr(),
                   fs.interpolate_bytes(C), flags, stream())
    torch.cuda.synchronize()
    return words(out)


def bwd(fs, vis, uv, gout, texs, modes, batch_slot, want=None, want_uv=True, flags=F, fill=SENTINEL, into=None, with_tex=True, share=None):
    """the backward pass → (per slot gtex float32 of the texture's shape — added into into[s] or zeros — or None where not wanted,
    guv uint32 [n, 2, rows, W] from `fill` or None)"""
    C, m, g = texs[0].shape[-1], map_dev(batch_slot), dev(gout)
    want = [True] * len(texs) if want is None else want
    t_dev = upload(texs, share) if with_tex else [None] * len(texs)
    gt = [(torch.zeros(t.shape, dtype=torch.float32, device="cuda") if into is None or into[s] is None else dev(into[s])) if want[s] else None
          for s, t in enumerate(texs)]
    gu = filled(fs.interpolate_shape(2), fill) if want_uv else None
    fs.texture_set_grad(vis.data_ptr(), uv.data_ptr(), g.data_ptr(), slot_tuples(texs, t_dev, modes, gt), m.data_ptr(), len(batch_slot), C,
                        gu.data_ptr() if want_uv else None, flags, stream())
    torch.cuda.synchronize()
    return [x.cpu().numpy() if x is not None else None for x in gt], (words(gu) if want_uv else None)


def check_gtex(got, accs, what, exact=False, init=None):
    """got: one slot's gtex; accs: its texref.Grads, one (a shared texture) or one per frame; init: what the buffer held before"""
    ref = np.stack([a.gtex for a in accs]).reshape(got.shape)
    mag = np.stack([a.gabs for a in accs]).reshape(got.shape)
    cnt = np.stack([np.broadcast_to(a.count[:, :, None], a.gtex.shape) for a in accs]).reshape(got.shape).astype(np.float64)
    if init is not None:
        ref, mag, cnt = ref + init.astype(np.float64), mag + np.abs(init.astype(np.float64)), cnt + 1
    assert np.isfinite(ref).all()
    nu = cnt * 2.0 ** -24
    bound = nu / (1.0 - nu) * mag
    if exact:
        assert (ref.astype(np.float32).astype(np.float64) == ref).all(), "the case is not dyadic"
        bound = np.zeros_like(bound)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}, "
          f"max n {int(cnt.max())}, elements with one add {int((cnt == 1).sum())}, untouched {int((cnt == 0).sum())}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, first {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4]} bound {bound[bad][:4]}"
    one = cnt == 1
    same((got + np.float32(0))[one], (ref.astype(np.float32) + np.float32(0))[one], what + " (n = 1)")
    assert (got[cnt == 0] == 0).all()


def owners(v, frames):
    return np.stack([((v[i, 1] & 0x7fffffff) - np.uint32(1)) < f.n_tris for i, f in enumerate(frames)])


def rand_gout(seed, shape, own=None):
    g = np.random.default_rng([seed, 8]).normal(0, 2, shape).astype(np.float32)
    if own is not None:
        g[np.broadcast_to(~own[:, None], g.shape)] = np.nan  # nobody's words may hold anything
    return g


def rendered(ctx, frames):
    fs = ctx.frameset(frames)
    vis = visibility(fs)
    v = words(vis)
    uv, uvw = interp_uv(fs, vis, frames)
    return fs, vis, v, uv, uvw, owners(v, frames)


def hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, modes, batch_slot, what, seed=1, gtex=True, share=None):
    """forward with and without the fused clear, guv, and (gtex) every slot's texel gradient within its bound, against texsetref"""
    C = texs[0].shape[-1]
    for flags in (F, 0):
        fused = bool((frames[0].c.flags | flags) & F)  # (frame flags | flags: a frame that clears is fused whatever the call says)
        got = fwd(fs, vis, uv, texs, modes, batch_slot, flags, share=share)
        same(got, texsetref.forward_set(tmp_path, frames, v, uvw, texs, modes, batch_slot, fused, SENTINEL), f"{what} flags {flags}")
        written = np.broadcast_to(own[:, None], got.shape)
        assert (got[written] != SENTINEL).all() and (got[~written] == (0 if fused else SENTINEL)).all(), what
    gout = rand_gout(seed, (len(frames), C) + v.shape[2:], own)
    gt, gu = bwd(fs, vis, uv, gout, texs, modes, batch_slot, want=None if gtex else [False] * len(texs), share=share)
    accs, want_gu = texsetref.grad_set(tmp_path, frames, v, uvw, gout, texs, modes, batch_slot, True, SENTINEL)
    same(gu, want_gu, what + " guv")
    assert (gu[np.broadcast_to(own[:, None], gu.shape)] != SENTINEL).all()
    if gtex:
        for s, g in enumerate(gt):
            check_gtex(g, accs.acc[s], f"{what} gtex slot {s}")
    return got, gu, gt, accs


# ------------------------------------------------------------------------------------------------------ forward and guv
def case_frames(name):
    if name in ("36x33", "70x33"):  # partial tiles, a width that is no multiple of 4 (70) and one that is (36)
        w, h = (36, 33) if name == "36x33" else (70, 33)
        back = ccw((w + 8, h + 8), (-16, h + 8), (w + 8, -19), z=80.0, uv=((0.1, 0.2), (0.9, 0.3), (0.4, 0.95)))  # (the upper left is left out)
        return [frame(split(np.concatenate([soup(1 + i, 40, w, h, ZS, big=True), back]), 3), w, h, flags=0) for i in range(2)]
    if name == "stack":
        return [frame(split(stack(50, jitter=i).tris[0], 3), 64, 64, flags=0) for i in range(2)]
    return [texsetref.three_frame(2, flags=0), texsetref.three_frame(5, flags=0)]  # (the frames do not clear: without the flag nobody's words stay)


@pytest.mark.parametrize("name", ["36x33", "70x33", "stack", "three"])
def test_forward_and_guv_frames_sizes_modes_and_channels(ctx, tmp_path, name):
    """textures of 1 x 1, 5 x 7, 33 x 1 and 64 x 64 in one call, CLAMP and WRAP mixed, shared and per frame mixed; 1, 3, 5 and 64
    channels; two maps over the three batches"""
    frames = case_frames(name)
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    assert own.sum() >= 300 and (~own).sum() >= 50
    wide = make_texs(3, 64, 2)
    modes = [CLAMP, WRAP, WRAP, CLAMP]
    for C in CHANNELS:
        texs = [np.ascontiguousarray(t[..., :C]) for t in wide]
        for batch_slot in ((3, 1, 0), (2, 0, 2)):
            hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, modes, batch_slot, f"{name} C {C} map {batch_slot}", seed=C, gtex=C == 5)
    fs.close()


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("name", ["70x33", "three"])
def test_two_slots_share_one_d_tex_with_different_modes(ctx, tmp_path, name, per_frame):
    """ONE device tensor is both slots' d_tex, clamped for batches 0 and 2 and wrapped for batch 1 (and the other way round), each
    slot with a d_gtex of its own; the uv reach far beyond [0, 1], where the two modes give different texels.  Forward and guv word
    for word, both slots' gtex within the bound; and the words are not those of the modes swapped: the mode is the slot's own"""
    frames = case_frames(name)
    fs, vis, v, _, uvw, own = rendered(ctx, frames)
    uvw = (uvw * np.float32(3) - np.float32(1)).astype(np.float32)  # [0, 1] -> [-1, 2]
    uv = dev(uvw)
    tex = texref.make_tex(6, 5, 7, 5, frames=2 if per_frame else None)
    texs, batch_slot = [tex, tex], (0, 1, 0)
    for modes in ([CLAMP, WRAP], [WRAP, CLAMP]):
        got, gu, gt, accs = hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, modes, batch_slot, f"shared d_tex {name} {modes}", share={1: 0})
        swapped = texsetref.forward_set(tmp_path, frames, v, uvw, texs, modes[::-1], batch_slot, False, SENTINEL).view(np.uint32)
        slots = np.stack([texsetref.slot_plane(frames[i], v[i, 1], batch_slot, 2) for i in range(2)])
        for s in (0, 1):  # in either slot's pixels the other mode would have given other words: both slots are told apart
            assert (got != swapped)[np.broadcast_to((slots == s)[:, None], got.shape)].sum() >= 50, (modes, s)
            assert sum(int(a.count.sum()) for a in accs.acc[s]) >= 4 * 100 and (gt[s] != 0).any()
        assert not np.array_equal(gt[0], gt[1])
    fs.close()


@pytest.mark.parametrize("n_slots,batch_slot", [(1, (0, 0, 0, 0, 0)), (2, (0, 1, 0, 1, 1)), (3, (1, 0, 2, 2, 0)), (8, (7, 0, 3, 5, 2))])
def test_slot_counts_and_a_second_launch(ctx, tmp_path, n_slots, batch_slot):
    frames = [texsetref.holes_frame(flags=0)] * 2
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    texs = make_texs(7, 3, 2, n=n_slots)
    modes = [(CLAMP, WRAP)[s % 2] for s in range(n_slots)]
    got, gu, _, accs = hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, modes, batch_slot, f"{n_slots} slots")
    for s in range(n_slots):  # the slots of the map are met, the others are not
        assert (sum(int(a.count.sum()) for a in accs.acc[s]) > 0) == (s in batch_slot), s
    assert np.array_equal(fwd(fs, vis, uv, texs, modes, batch_slot, 0), got)  # (hold's last forward: without the fused clear)
    gout = rand_gout(1, (2, 3) + v.shape[2:], own)
    assert np.array_equal(bwd(fs, vis, uv, gout, texs, modes, batch_slot, want=[False] * n_slots)[1], gu)
    fs.close()


def test_a_map_with_none_a_short_map_and_a_byte_that_names_no_slot(ctx, tmp_path):
    frames = [texsetref.holes_frame(flags=0)] * 2
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    texs, modes = make_texs(9, 5, 2, n=3), [WRAP, CLAMP, WRAP]
    b = np.stack([texsetref.batch_plane(frames[i], v[i, 1]) for i in range(2)])
    unsampled = (b == 2) | (b == 4)
    assert (b == 2).sum() >= 100 and (b == 4).sum() >= 100
    res = []
    for batch_slot in (texsetref.HOLES_MAP, texsetref.HOLES_MAP_200):
        got, gu, gt, _ = hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, modes, batch_slot, f"map {batch_slot}")
        for a in (got, gu):  # owned and unsampled: zeros, written
            assert (a[np.broadcast_to(unsampled[:, None], a.shape)] == 0).all()
        res.append((got, gu))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    fs.close()


def test_uv_that_are_not_finite(ctx, tmp_path):
    f = texref.case_frame("uv-nonfinite")
    frames = [f, f]
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    assert (~np.isfinite(uvw).all(1) & own).sum() >= 40
    batch_slot = (1, 0)
    b = texsetref.batch_plane(f, v[0, 1])
    assert len(f.tris) == 2 and (b == 0).sum() >= 100 and (b == 1).sum() >= 100
    hold(tmp_path, fs, vis, v, uv, uvw, own, frames, make_texs(11, 3, 2, n=2), [CLAMP, WRAP], batch_slot, "uv-nonfinite")
    fs.close()


# ------------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("mode", [CLAMP, WRAP])
def test_one_slot_is_srz_frameset_texture_on_the_device(ctx, mode):
    frames = case_frames("three")
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    tex = texref.make_tex(2, 5, 7, 5, frames=2)
    t, C = dev(tex), 5
    out, gu = filled(fs.interpolate_shape(C)), filled(fs.interpolate_shape(2))
    gout = rand_gout(4, (2, C) + v.shape[2:], own)
    g, gt = dev(gout), torch.zeros_like(t)
    fs.texture(vis.data_ptr(), uv.data_ptr(), t.data_ptr(), 5, 7, C, 2, mode, out.data_ptr(), fs.interpolate_bytes(C), 0, stream())
    fs.texture_grad(vis.data_ptr(), uv.data_ptr(), g.data_ptr(), t.data_ptr(), 5, 7, C, 2, mode, gt.data_ptr(), gu.data_ptr(), 0, stream())
    torch.cuda.synchronize()
    assert np.array_equal(fwd(fs, vis, uv, [tex], [mode], (0, 0, 0), 0), words(out))
    gts, gus = bwd(fs, vis, uv, gout, [tex], [mode], (0, 0, 0), flags=0)
    assert np.array_equal(gus, words(gu))
    assert np.allclose(gts[0], gt.cpu().numpy(), rtol=0, atol=1e-3) and (gts[0] != 0).any()  # (both are atomic sums: held to the bound elsewhere)
    fs.close()


def test_a_sceneset_of_two_draws_slot_by_draw(ctx, tmp_path):
    w = h = 64
    draws = []
    for i in range(2):
        verts, faces = unshared_mesh(soup(5 + 2 * i, 40, w, h, ZS, big=True), w, h, 30 + i)
        draws.append((verts, faces, abi.SHADER_NORMAL, -1, place(w, h, 0.0, 0.0), IDENT))
    sf, f = scene_pair(draws, w, h, (0.0, 0.0, 1.0), [], 1.0, 0.0, ctx=ctx, slots=[40, 41])
    fs = ctx.frameset([sf])
    vis = visibility(fs)
    v = words(vis)
    uv, uvw = interp_uv(fs, vis, [f])
    own = owners(v, [f])
    b = texsetref.batch_plane(f, v[0, 1])
    assert (b == 0).sum() >= 200 and (b == 1).sum() >= 200
    texs, modes = [texref.make_tex(1, 5, 7, 3), texref.make_tex(2, 64, 64, 3)], [WRAP, CLAMP]
    got = hold(tmp_path, fs, vis, v, uv, uvw, own, [f], texs, modes, (1, 0), "sceneset")[0]
    # the set of the same triangles as batches: the same words
    fs2 = ctx.frameset([f])
    vis2 = visibility(fs2)
    assert np.array_equal(words(vis2), v)
    assert np.array_equal(fwd(fs2, vis2, uv, texs, modes, (1, 0), 0), got)
    fs.close(), fs2.close()


# ------------------------------------------------------------------------------------------------------ gtex
def pow2_gout(seed, shape):
    rng = np.random.default_rng([seed, 3])
    return (rng.choice(np.float32([-1, 1]), shape) * 2.0 ** rng.integers(0, 5, shape)).astype(np.float32)


def test_gtex_exact_on_dyadic_inputs_where_two_slots_share_texel_indices(ctx, tmp_path):
    """the shared-index case: both slots' textures are 8 x 8, every pixel lies on a texel centre, gout are small powers of two, the
    buffers added into hold integers — every partial sum is representable, so each slot's gradient is exact in any order of adds; a
    table keyed on the texel index alone would move one slot's adds into the other's texture"""
    frames = [texsetref.shared_frame()] * 2
    fs, vis, v, _, _, own = rendered(ctx, frames)
    tw, th = texsetref.SHARED_TEX
    uvw = texsetref.centre_uv(1, 2, 64, 64, tw, th)
    uv = dev(uvw)
    rng = np.random.default_rng(17)
    for C in (1, 5):
        texs = [rng.integers(-8, 9, (th, tw, C)).astype(np.float32), rng.integers(-8, 9, (2, th, tw, C)).astype(np.float32)]
        modes, batch_slot = [CLAMP, WRAP], (0, 1)
        gout = pow2_gout(C, (2, C, 64, 64))
        init = [rng.integers(-64, 65, t.shape).astype(np.float32) for t in texs]
        gt, gu = bwd(fs, vis, uv, gout, texs, modes, batch_slot, into=init)
        accs, want_gu = texsetref.grad_set(tmp_path, frames, v, uvw, gout, texs, modes, batch_slot, True, SENTINEL)
        same(gu, want_gu, "dyadic guv")
        for s in (0, 1):
            check_gtex(gt[s], accs.acc[s], f"dyadic C {C} slot {s}", exact=True, init=init[s])
            assert (gt[s] != init[s]).any()
        assert not np.array_equal(accs.acc[0][0].gtex, accs.acc[1][0].gtex)  # the slots' sums differ: a merge would show
        same(fwd(fs, vis, uv, texs, modes, batch_slot), texsetref.forward_set(tmp_path, frames, v, uvw, texs, modes, batch_slot, True, SENTINEL), "dyadic forward")
    fs.close()


def test_gtex_where_the_pairs_of_a_tile_overflow_the_table(ctx, tmp_path):
    """the overflow case: each slot's texels of tile (0, 0) fit the table, the two slots' together do not — corners that find no entry
    add straight to memory, into their own slot's texture"""
    frames = [texsetref.overflow_frame()] * 2
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    slots = texsetref.slot_plane(frames[0], v[0, 1], (0, 1), 2)
    n = [len(texsetref.touched(tmp_path, frames[0], (64, 64), CLAMP, v[0, 1], uvw[0], slots, s, (0, 0))) for s in (0, 1)]
    assert max(n) <= texsetref.TG_SLOTS < sum(n), n
    texs = [texref.make_tex(1, 64, 64, 5), texref.make_tex(2, 64, 64, 5, frames=2)]
    hold(tmp_path, fs, vis, v, uv, uvw, own, frames, texs, [CLAMP, CLAMP], (0, 1), "overflow")
    fs.close()


def test_gtex_null_beside_one_accumulation_and_a_slot_nobody_maps_to(ctx, tmp_path):
    frames = case_frames("three")
    fs, vis, v, uv, uvw, own = rendered(ctx, frames)
    C = 3
    texs = make_texs(5, C, 2, n=3) + [np.full((7, 5, C), np.nan, np.float32)]  # slot 3: nobody maps to it; its texels are NaN throughout
    modes, batch_slot = [WRAP, CLAMP, WRAP, WRAP], texsetref.THREE_MAP
    gout = rand_gout(2, (2, C) + v.shape[2:], own)
    init = [np.random.default_rng(4).normal(0, 5, texs[0].shape).astype(np.float32), None, None, None]
    gt, gu = bwd(fs, vis, uv, gout, texs, modes, batch_slot, want=[True, False, True, True], into=init)
    accs, want_gu = texsetref.grad_set(tmp_path, frames, v, uvw, gout, texs[:3], modes[:3], batch_slot, True, SENTINEL)
    same(gu, want_gu, "guv beside a NaN slot")
    assert not np.isnan(gu.view(np.float32)[np.broadcast_to(own[:, None], gu.shape)]).any()
    check_gtex(gt[0], accs.acc[0], "into a non-zero buffer", init=init[0])
    assert gt[1] is None
    check_gtex(gt[2], accs.acc[2], "beside a slot without gtex")
    assert (gt[3].view(np.uint32) == 0).all()  # not one add, not a -0
    same(fwd(fs, vis, uv, texs, modes, batch_slot), texsetref.forward_set(tmp_path, frames, v, uvw, texs[:3], modes[:3], batch_slot, True, SENTINEL),
         "forward beside a NaN slot")
    # gtex alone needs no texture: d_tex null in every slot, d_guv null
    only, none = bwd(fs, vis, uv, gout, texs, modes, batch_slot, want=[True, True, True, False], want_uv=False, with_tex=False)
    assert none is None and only[3] is None
    for s in range(3):
        check_gtex(only[s], accs.acc[s], f"gtex alone, slot {s}")
    fs.close()
