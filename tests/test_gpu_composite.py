"""-m gpu: srz_frameset_composite / _composite_grad (k_composite, k_composite_grad) against tests/compositeref.py's binary32
reference, bit for bit (NaN for NaN): the forward and every gradient plane, on frames with a partial tile column and band, on a width
that is no multiple of four, and on triangles stacked over one tile; 1 to 8 layers (both builds of the kernels: up to 4 layers and up
to 8), 1 to 64 channels, alpha as plane and as scalar, with and without the background and the transmittance plane, every subset of
the gradient outputs, layers that are not a peel chain, hostile alphas, NaN wherever a layer does not cover — and the forward against
the existing torch composite on the device."""
import itertools
import types

import numpy as np
import pytest
import torch

import compositeref as cr
from srz import abi
from srz import visibility as V
from support import SENTINEL, ccw, ctx, filled, frame, soup, stack, words  # noqa: F401  (ctx: the fixture)
from walkkit import same

pytestmark = pytest.mark.gpu

ZS = np.float32([1, 2, 3, 4])
GEOMETRIES = ("36x33", "70x33", "stack")


def frames_of(name):
    """stack: support.stack's triangles over one tile, enough of them that three lie over one pixel whichever half the cull keeps.
    Else two frames of a small soup in front of four staggered triangles, each of which covers the lower right of the frame (the
    partial tile column, the partial band) and leaves the upper left corner to the soup and to nobody"""
    if name == "stack":
        return [stack(24, jitter=2), stack(32), stack(40, jitter=1)]
    w, h = (36 if name == "36x33" else 70), 33
    out = []
    for seed in (3, 4):
        back = [ccw((w + 8, h + 8), (-16 - 6 * i - seed, h + 8), (w + 8, -19 - 5 * i), z=10.0 * (i + 1)) for i in range(4)]
        out.append(frame(np.concatenate([soup(seed, 8, w, h, ZS)] + back), w, h))
    return out


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def worlds(ctx, tmp_path_factory):
    """per geometry: the set, its first eight depth layers on the device, their id words and coverage — made on first use"""
    tmp, made = tmp_path_factory.mktemp("compositeref"), {}

    def get(name):
        if name in made:
            return made[name]
        frames = frames_of(name)
        w = types.SimpleNamespace(name=name, tmp=tmp, fs=ctx.frameset(frames), n_tris=[f.n_tris for f in frames])
        w.layers = V.layers(w.fs, 8)
        torch.cuda.synchronize()
        # from decode alone: each of layers 1-3 owns pixels in every frame, and some pixel is covered by all three
        own = [(V.decode(t).tri >= 0).cpu().numpy() for t in w.layers]
        for k in range(3):
            assert own[k].reshape(len(frames), -1).any(1).all(), (name, k)
        assert (own[0] & own[1] & own[2]).reshape(len(frames), -1).any(1).all(), name
        assert not own[0].all() and (~own[0] & ~own[1] & ~own[2]).any(), name  # (and some pixel by none)
        w.ids = [words(t)[:, 1] for t in w.layers]
        w.cov = [cr.cover(tmp, i, w.n_tris) for i in w.ids]
        for k in range(8):
            assert np.array_equal(w.cov[k], own[k]), (name, k)  # (the reference's owner test and decode's agree on peeled layers)
        made[name] = w
        return w
    yield get
    for w in made.values():
        w.fs.close()


HOSTILE_ALPHAS = np.float32([0, 1, 2, -1, np.inf, np.nan])


def make_inputs(w, order, n_ch, scalar, with_bg, hostile, seed):
    """the layers `order` (indices into the world's eight) with random colours and alphas, NaN wherever the layer does not cover;
    hostile: a third of the covering alphas drawn from 0, 1, 2, -1, inf, NaN → a namespace of host arrays"""
    rng = np.random.default_rng([seed, n_ch, len(order)])
    n, _, rows, W = w.fs.out_shape
    c = types.SimpleNamespace(order=list(order), n_ch=n_ch, covs=[w.cov[k] for k in order], colors=[], alphas=[])
    for i, k in enumerate(order):
        cv = w.cov[k][:, None]
        col = rng.uniform(-1, 2, (n, n_ch, rows, W)).astype(np.float32)
        c.colors.append(np.where(cv, col, np.float32(np.nan)).astype(np.float32))
        if i in scalar:
            c.alphas.append(float(HOSTILE_ALPHAS[i % 4]) if hostile else float(np.float32(rng.uniform(0, 1))))
        else:
            a = rng.uniform(0, 1, (n, 1, rows, W)).astype(np.float32)
            if hostile:
                pick = rng.integers(0, 3 * len(HOSTILE_ALPHAS), a.shape)
                a = np.where(pick < len(HOSTILE_ALPHAS), HOSTILE_ALPHAS[pick % len(HOSTILE_ALPHAS)], a).astype(np.float32)
            c.alphas.append(np.where(cv, a, np.float32(np.nan)).astype(np.float32))
    c.bg = rng.uniform(-1, 2, (n, n_ch, rows, W)).astype(np.float32) if with_bg else None
    return c


def on_device(w, c):
    lay = [w.layers[k] for k in c.order]
    cols = [dev(x) for x in c.colors]
    als = [a if np.isscalar(a) else dev(a) for a in c.alphas]
    return lay, cols, als, None if c.bg is None else dev(c.bg)


def raw_forward(w, c, lay, cols, als, bg, through):
    """FrameSet.composite into a sentinel-filled buffer → its words"""
    planes = c.n_ch + (1 if through else 0)
    out = filled(w.fs.interpolate_shape(planes))
    tup = [(lay[i].data_ptr(), cols[i].data_ptr(), None if np.isscalar(als[i]) else als[i].data_ptr(), als[i] if np.isscalar(als[i]) else 0.0)
           for i in range(len(lay))]
    w.fs.composite(tup, c.n_ch, None if bg is None else bg.data_ptr(), through, out.data_ptr(), out.numel() * 4, abi.FUSED_CLEAR,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return words(out), tup


def raw_grad(w, c, tup, bg, through, gout, want_c, want_a, want_bg):
    """FrameSet.composite_grad into sentinel-filled buffers → (gcolor words or None per layer, galpha likewise, gbg words or None)"""
    n = len(tup)
    gc = [filled(w.fs.interpolate_shape(c.n_ch)) if want_c[i] else None for i in range(n)]
    ga = [filled(w.fs.interpolate_shape(1)) if want_a[i] else None for i in range(n)]
    gb = filled(w.fs.interpolate_shape(c.n_ch)) if want_bg else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    w.fs.composite_grad(tup, c.n_ch, ptr(bg), through, gout.data_ptr(), [ptr(t) for t in gc], [ptr(t) for t in ga], ptr(gb),
                        abi.FUSED_CLEAR, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wd = lambda t: None if t is None else words(t)  # noqa: E731
    return [wd(t) for t in gc], [wd(t) for t in ga], wd(gb)


def no_sentinel(a, what):
    assert not (a == SENTINEL).any(), f"{what}: a sentinel survives"


def check_case(w, c, through, subsets, seed=0):
    """forward and gradients of one set of inputs against the reference; subsets: (want_gcolor, want_galpha, want_gbg) triples"""
    lay, cols, als, bg = on_device(w, c)
    got, tup = raw_forward(w, c, lay, cols, als, bg, through)
    want = cr.forward(w.tmp, c.covs, c.colors, c.alphas, c.bg, through)
    what = f"{w.name} L={len(c.order)} C={c.n_ch} bg={c.bg is not None} T={through}"
    no_sentinel(got, what)
    same(got, want, what + " forward")
    rng = np.random.default_rng([seed, 99])
    g = rng.uniform(-1, 1, want.shape).astype(np.float32)
    gcol, galpha, gbg = cr.grad(w.tmp, c.covs, c.colors, c.alphas, g, c.bg, through)
    g_dev = dev(g)
    for want_c, want_a, want_bg in subsets:
        rc, ra, rb = raw_grad(w, c, tup, bg, through, g_dev, want_c, want_a, want_bg)
        for i in range(len(c.order)):
            for r, ref, kind in ((rc[i], gcol[i], "gcolor"), (ra[i], galpha[i], "galpha")):
                if r is not None:
                    no_sentinel(r, f"{what} {kind}[{i}]")
                    same(r, ref, f"{what} {kind}[{i}] of {want_c, want_a, want_bg}")
                    assert not r[np.broadcast_to(~c.covs[i][:, None], r.shape)].any(), f"{what} {kind}[{i}]: not +0 where the layer does not cover"
        if rb is not None:
            no_sentinel(rb, what + " gbg")
            same(rb, gbg, what + " gbg")
    return got, want


def all_of(n, bg):
    return [([True] * n, [True] * n, bg)]


# (n_layers, n_ch, the layers with a scalar opacity, background, transmittance plane): every count of layers on both sides of the
# kernels' two builds (up to 4 and up to 8 layers), every channel count on both sides of the register chunk of 4
SHAPES = [(1, 1, (), False, False), (1, 3, (0,), True, True), (2, 3, (1,), True, False), (3, 5, (0, 2), False, True), (3, 3, (), True, True),
          (4, 3, (3,), True, True), (5, 1, (1, 4), True, False), (8, 3, (2, 5), True, True), (8, 5, (), False, False), (3, 64, (1,), True, True),
          (8, 64, (0, 7), True, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"L{s[0]}-C{s[1]}-s{len(s[2])}-bg{int(s[3])}-T{int(s[4])}")
@pytest.mark.parametrize("name", GEOMETRIES)
def test_forward_and_gradients_are_the_reference(worlds, name, shape):
    n_layers, n_ch, scalar, with_bg, through = shape
    w = worlds(name)
    c = make_inputs(w, range(n_layers), n_ch, scalar, with_bg, False, 1)
    check_case(w, c, through, all_of(n_layers, with_bg))


@pytest.mark.parametrize("name", GEOMETRIES)
def test_every_subset_of_the_gradient_outputs(worlds, name):
    """the seven non-empty subsets of {gcolor, galpha, gbg} with every layer asked alike, then per-layer masks: colours of the even
    layers with alphas of the odd ones, one single plane, and galpha of a layer whose alpha is the scalar"""
    w = worlds(name)
    c = make_inputs(w, range(3), 3, (1,), True, False, 2)
    subsets = [([a] * 3, [b] * 3, g) for a, b, g in itertools.product((False, True), repeat=3) if a or b or g]
    subsets += [([True, False, True], [False, True, False], False), ([False, False, False], [False, False, True], False),
                ([False, True, False], [False, False, False], False), ([False, False, False], [False, True, False], True)]
    check_case(w, c, True, subsets)
    c = make_inputs(w, range(3), 5, (), False, False, 3)  # (without a background: no gbg to ask for)
    check_case(w, c, False, [([True] * 3, [False] * 3, False), ([False] * 3, [True] * 3, False), ([True, False, False], [False, False, True], False)])


@pytest.mark.parametrize("name", GEOMETRIES)
def test_layers_that_are_not_a_peel_chain(worlds, name):
    """the same buffer twice, the order reversed, an empty layer in the middle and in front"""
    w = worlds(name)
    for order, scalar in (((0, 0), ()), ((2, 1, 0), (1,)), ((0, 7, 1, 7, 2), (3,)), ((7, 6, 0, 1, 1, 2, 0, 5), (0, 4))):
        c = make_inputs(w, order, 3, scalar, True, False, 4)
        check_case(w, c, True, all_of(len(order), True))


@pytest.mark.parametrize("name", GEOMETRIES)
def test_hostile_alphas_and_nan_wherever_a_layer_does_not_cover(worlds, name):
    """alpha 0, 1, 2, -1, inf and NaN at covering pixels, as plane words and as scalars; NaN in every word of a colour or alpha plane
    at pixels its layer does not cover (make_inputs), which must not reach any result"""
    w = worlds(name)
    for n_layers, scalar in ((3, ()), (3, (0, 1, 2)), (8, (3,))):
        c = make_inputs(w, range(n_layers), 3, scalar, True, True, 5)
        for a, cv in zip(c.alphas[:3], c.covs[:3]):  # (the layers every frame has)
            if not np.isscalar(a):
                for v in HOSTILE_ALPHAS[:5]:
                    assert (a[cv[:, None]] == v).any(), v
                assert np.isnan(a[cv[:, None]]).any() and np.isnan(a[~cv[:, None]]).all()
        got, want = check_case(w, c, True, all_of(n_layers, True))
        none = ~np.logical_or.reduce(c.covs)
        assert none.any() and (got[:, 3][none] == np.float32(1).view(np.uint32)).all()  # nobody's pixels: T = 1, the colour is bg
        assert np.array_equal(got[:, :3][np.broadcast_to(none[:, None], got[:, :3].shape)],
                              (c.bg + np.float32(0)).view(np.uint32)[np.broadcast_to(none[:, None], c.bg.shape)])


@pytest.mark.parametrize("name", GEOMETRIES)
def test_forward_is_the_torch_composite_on_finite_inputs(worlds, name):
    """composite(colors, [alpha_k * coverage_k]) (+ through * bg) run on the device, as float values with +-0 alike"""
    w = worlds(name)
    for n_layers, n_ch, scalar, with_bg in ((1, 3, (), False), (3, 3, (1,), True), (8, 5, (0,), True)):
        c = make_inputs(w, range(n_layers), n_ch, scalar, with_bg, False, 6)
        lay, cols, als, bg = on_device(w, c)
        out = V.composite_layers(w.fs, lay, cols, als, bg, through=True)
        cov = [torch.as_tensor(cv[:, None]).cuda() for cv in c.covs]
        zero = torch.zeros((), device="cuda")
        cols0 = [torch.where(cv, x, zero) for cv, x in zip(cov, cols)]  # (the torch loop multiplies every word: no NaN may be there)
        eff = [torch.where(cv, a if torch.is_tensor(a) else torch.full_like(cols[0][:, :1], a), zero) for cv, a in zip(cov, als)]
        ref = V.composite(cols0, eff)
        T = torch.ones_like(eff[0])
        for e in eff:
            T = T * (1 - e)
        if bg is not None:
            ref = ref + T * bg
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out[:, :n_ch], ref) and torch.equal(out[:, n_ch:], T), (name, n_layers, n_ch)  # (== : +0 and -0 alike)


def test_a_second_launch_gives_the_same_words(worlds):
    w = worlds("36x33")
    c = make_inputs(w, range(3), 3, (), True, False, 7)
    lay, cols, als, bg = on_device(w, c)
    a, tup = raw_forward(w, c, lay, cols, als, bg, True)
    b, _ = raw_forward(w, c, lay, cols, als, bg, True)
    assert np.array_equal(a, b)
    g = dev(np.random.default_rng(8).uniform(-1, 1, a.shape))
    x = raw_grad(w, c, tup, bg, True, g, [True] * 3, [True] * 3, True)
    y = raw_grad(w, c, tup, bg, True, g, [True] * 3, [True] * 3, True)
    for p, q in zip(x[0] + x[1] + [x[2]], y[0] + y[1] + [y[2]]):
        assert np.array_equal(p, q)
