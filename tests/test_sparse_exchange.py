"""not-gpu: the tile-sparse exchange (srz_frameset_sparse_*, srz_frameset_allgather_sparse).

The C ABI declares and exports it; the header's band map is the one the code ships; the kernels' touched test is k_clear's; and the
protocol — header all-gather, padded all-gather of the messages, unpack — run through the torch formulation (srz.parallel) over gloo
with world 2 and 3 reassembles the oracle's frames bit for bit while sending fewer bytes than the dense shard."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srz.h")
KERNELS = os.path.join(REPO, "software-rasterizer_amd", "csrc", "srz_kernels.hip")
SPARSE = ("srz_frameset_sparse_capacity", "srz_frameset_sparse_pack", "srz_frameset_sparse_unpack", "srz_frameset_allgather_sparse")


def test_header_declares_and_library_exports_the_sparse_entry_points():
    import srz
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in SPARSE:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in srz.EXPORTS, name


def test_header_band_map_is_the_shipped_one():
    """the header states rank(b) as a formula; evaluated as written it must be parallel.rank_of_band (= csrc/srz_device.h)"""
    from srz import parallel
    text = open(HEADER).read()
    m = re.search(r"rank\(b\) = (\(b \+ band_rot\(world\) \* \(b / world\)\) % world),\s*band_rot\(world\) = (\d+), or (\d+) when (\d+) % world == 0",
                  text)
    assert m, "srz.h does not state the band map rank(b) = ... with band_rot(world)"
    expr, rot, rot_alt, mod = m.group(1).replace("/", "//"), int(m.group(2)), int(m.group(3)), int(m.group(4))
    assert "b % world == rank" not in text and "rank (y / 32) % world" not in text   # (the pre-rotation map of rounds 1-5)
    for world in (2, 3, 5, 8, 10):
        band_rot = (lambda w: rot_alt if mod % w == 0 else rot)  # noqa: E731  (world 10: 5 steps; world 5: 1)
        for b in range(4 * world * world):
            got = eval(expr, {"b": b, "world": world, "band_rot": band_rot})  # noqa: S307  (the header's own formula)
            assert got == parallel.rank_of_band(b, world), (world, b)


def _body(src, name):
    i = src.index(name)
    return src[i: src.index("\n}\n", i)]


def test_touched_test_is_k_clears():
    """k_sparse_pack's touched test is a copy of the one k_clear uses to leave a tile alone (k_clear itself is tuned and not
    shared): same render-flags test, same tile-count test on the same tile_info row"""
    src = open(KERNELS).read()
    clear, sparse = _body(src, "void k_clear(RenderArgs a)"), _body(src, "bool sparse_touched(")
    assert "if (!((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR)) continue;" in clear
    assert "if (!((fd->flags | a.flags_or) & SRZ_FUSED_CLEAR)) return true;" in sparse
    assert "if (cnt[(uint32_t)x4 / TILE].x != 0u) continue;" in clear
    assert "return cnt[tx].x != 0u;" in sparse
    row = "as_const(reinterpret_cast<const u32x2 *>(a.tile_info)) + "
    assert row + "(size_t)br * a.tiles_x;" in clear and "br = it >> 2" in clear
    assert row + "((size_t)f * a.n_local_bands + lb) * a.tiles_x;" in sparse


def test_formulation_round_trip_with_a_superset_and_odd_sizes():
    """one process plays every rank: pack with an over-full touched set, unpack — the frames come back, padding rows untouched"""
    from srz import parallel
    world, h, w = 3, 70, 37
    g = torch.Generator().manual_seed(5)
    lay = [parallel.shard_layout(h, r, world) for r in range(world)]
    shards = []
    for r in range(world):
        s = torch.zeros((2, 4, lay[r]["local_rows"], w), dtype=torch.float32)
        s[:, 0] = float("inf")
        s[:, :, 3:9, 30:35] = torch.rand((2, 4, 6, 5), generator=g)
        shards.append(s)
    gathered = torch.full((world,) + tuple(shards[0].shape), -5.0)
    msgs = []
    for r in range(world):
        touched = parallel.nonclear_tiles(shards[r], r, world, h)
        touched[0, 0, 0] = True                                    # a listed tile that is all clear: still valid
        msgs.append(parallel.sparse_pack(shards[r], touched, world, r, h))
        assert parallel.sparse_header(msgs[-1])[2] == msgs[-1].numel()
    for r in range(world):
        g2 = gathered.clone()
        g2[r] = shards[r]
        parallel.sparse_unpack(msgs, g2, r, world, h)
        for q in range(world):
            real = torch.zeros(lay[q]["local_rows"], dtype=torch.bool)
            for (lb, _, r0, r1) in parallel.band_rows(h, q, world):
                real[lb * 32: lb * 32 + r1 - r0] = True
            assert torch.equal(g2[q][:, :, real].view(torch.int32), shards[q][:, :, real].view(torch.int32)), (r, q)
            if q != r:   # padding rows (no band behind them) are not written
                assert (g2[q][:, :, ~real] == -5.0).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, height, width, q):
    import conftest  # noqa: F401
    import scenes
    from oracle import oracle
    from srz import parallel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        oracle.texture_set(scenes.TEX_SPOT, scenes.spot_texture())
        frames = [scenes.config2(i, size=width) if height == width else scenes.config3(i, width, height) for i in (1, 4)]
        lay = parallel.shard_layout(height, rank, world)
        shard = torch.zeros((len(frames), 4, lay["local_rows"], width), dtype=torch.float32)
        full_ref = []
        for fi, f in enumerate(frames):
            planes = oracle.new_planes(width, height)
            for (lb, band, r0, r1) in parallel.band_rows(height, rank, world):
                assert oracle.draw_rows(f, planes, r0, r1) == 0
                for p in range(4):
                    shard[fi, p, lb * 32: lb * 32 + (r1 - r0)] = torch.from_numpy(planes[p][r0:r1])
            full_ref.append(np.stack(oracle.draw(f)[1]))
        ok, sizes = True, []

        def check(g, kind):
            good = True
            for fi in range(len(frames)):
                for p in range(g.shape[2]):
                    for y in range(height):
                        row = parallel.gathered_row(g, fi, p, y, world).numpy()
                        ref = full_ref[fi][p][y] if kind == "planes" else ref8[fi, 0, y].numpy()
                        good = good and np.array_equal(row.view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))
            return good

        def to_bgr8(planes_f32):  # display()'s resolve (round half to even, saturate) as in test_shard_gloo.py
            c = torch.nan_to_num(planes_f32[:, 1:4], nan=0.0).round().clamp(0, 255).to(torch.uint8)
            return c.permute(0, 2, 3, 1).reshape(c.shape[0], 1, c.shape[2], -1).contiguous()
        ref8 = to_bgr8(torch.from_numpy(np.stack(full_ref)))
        for kind, s in (("planes", shard), ("bgr8", to_bgr8(shard))):
            touched = parallel.nonclear_tiles(s, rank, world, height)
            msg = parallel.sparse_pack(s, touched, world, rank, height)
            g = torch.zeros((world,) + tuple(s.shape), dtype=s.dtype)
            g[rank] = s
            g, m = parallel.all_gather_sparse(msg, g, rank, world, height)
            ok = ok and check(g, kind) and msg.numel() < s.numel() * s.element_size() and 0 < int(touched.sum()) < touched.numel()
            sizes.append((kind, msg.numel(), s.numel() * s.element_size(), m))
        q.put((rank, ok, sizes))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,height,width", [(2, 256, 256), (3, 200, 322)])
def test_sparse_protocol_over_gloo_reassembles_the_oracle(world, height, width):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, height, width, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == list(range(world))
    assert all(r[1] for r in res), res
