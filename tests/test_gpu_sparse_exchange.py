"""-m gpu: the tile-sparse exchange behind the C ABI (srz_frameset_sparse_capacity / _pack / _unpack, srz_frameset_allgather_sparse).

One GPU plays every rank: each rank renders its band shard into its own slot of its own gathered buffer and packs its message; the
messages are stacked at stride `capacity` (what a padded all-gather leaves) and every rank unpacks.  Every rank must then hold the
oracle's frames bit for bit, the same bytes as the dense in-place exchange, and the kernel's messages must be the torch formulation's
(srz.parallel.sparse_pack) given the kernel's own table.  The RCCL call runs at world 1 here and at world 2 when two GPUs are visible."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

import scenes
from srz import abi, parallel
from support import bits

pytestmark = pytest.mark.gpu
KINDS = (abi.EXCHANGE_PLANES, abi.EXCHANGE_BGR8)


def spot(i, w, h, flags=abi.FUSED_CLEAR):
    """config 2 (spot, TEXTURE) at any frame size"""
    tris = scenes.mesh_stream(scenes.SPOT_OBJ, w, h, float((10 * i) % 360), (0, 0, 0), 0.3)
    return abi.Frame(w, h, scenes.EYE, scenes.LIGHTS, [(abi.SHADER_TEXTURE, scenes.TEX_SPOT, tris)], flags)


def msg_table(msg, n_tab, shape):
    return msg[16: 16 + 4 * n_tab].clone().view(torch.int32).reshape(shape)


class Ranks:
    """every rank r of `world`: its ctx and set, its gathered buffer [world][frames][planes][local_rows][row] with its own shard
    rendered (FUSED_CLEAR unless flags say otherwise) or resolved into slot r, and its packed message (capacity bytes)"""

    def __init__(self, frames, world, what, flags=abi.FUSED_CLEAR, prefill=None):
        import srz
        self.world, self.what, self.h, self.w = world, what, frames[0].height, frames[0].width
        self.ctx, self.fs, self.g, self.msg = [], [], [], []
        s = torch.cuda.current_stream().cuda_stream
        for r in range(world):
            ctx = srz.Context(0, r, world)
            ctx.texture_upload(0, scenes.spot_texture())
            fs = ctx.frameset(frames)
            planes = torch.zeros((world,) + fs.out_shape, dtype=torch.float32, device="cuda")
            if prefill is not None:
                planes.fill_(prefill)
            fs.render(planes[r].data_ptr(), fs.out_bytes, flags, s)
            if what == abi.EXCHANGE_PLANES:
                g = planes
            else:
                g = torch.zeros((world, len(frames), 1, fs.local_rows, self.w * 3), dtype=torch.uint8, device="cuda")
                fs.resolve8(planes[r].data_ptr(), g[r].data_ptr(), g[r].numel(), s)
            cap = fs.sparse_capacity(what)
            msg = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
            fs.sparse_pack(g[r].data_ptr(), msg.data_ptr(), cap, what, s)
            self.ctx.append(ctx), self.fs.append(fs), self.g.append(g), self.msg.append(msg)
        torch.cuda.synchronize()
        self.cap = cap
        self.bpr = self.fs[0].local_rows // 32 if world > 1 else (self.h + 31) // 32
        self.lay = parallel.sparse_layout(len(frames), self.bpr, self.w, 4 if what == abi.EXCHANGE_PLANES else 1)

    def header(self, r):
        return parallel.sparse_header(self.msg[r])

    def table(self, r):
        return msg_table(self.msg[r], self.lay["n_tab"], (len(self.fs[0].frames), self.bpr, self.lay["tiles_x"]))

    def unpack_all(self):
        recv = torch.stack(self.msg).contiguous()     # = the padded all-gather at stride `capacity`
        s = torch.cuda.current_stream().cuda_stream
        for r in range(self.world):
            self.fs[r].sparse_unpack(recv.data_ptr(), self.cap, self.g[r].data_ptr(), self.what, s)
        torch.cuda.synchronize()

    def dense(self):
        """the dense in-place exchange's result: every rank's own slot"""
        return torch.stack([self.g[r][r] for r in range(self.world)])

    def real_rows(self, q):
        real = torch.zeros(self.g[0].shape[3], dtype=torch.bool, device="cuda")
        for (lb, _, r0, r1) in parallel.band_rows(self.h, q, self.world):
            real[lb * 32: lb * 32 + r1 - r0] = True
        return real

    def assert_equals_dense(self, dense):
        for r in range(self.world):
            for q in range(self.world):
                rr = self.real_rows(q)
                a, b = self.g[r][q][:, :, rr], dense[q][:, :, rr]
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (self.world, self.what, r, q)

    def close(self):
        for f, c in zip(self.fs, self.ctx):
            f.close(), c.close()


@pytest.mark.parametrize("world,w,h", [(2, 256, 256), (3, 101, 200), (8, 322, 270)])
def test_sparse_exchange_one_gpu_plays_every_rank(orc, world, w, h):
    frames = [spot(i, w, h) for i in (2, 11, 25)]
    refs = [np.stack(orc.draw(f)[1]) for f in frames]
    for what in KINDS:
        R = Ranks(frames, world, what)
        dense = R.dense().clone()
        for r in range(world):   # the kernel's message = the torch formulation given the kernel's own table
            n_t, n_tab, nbytes = R.header(r)
            assert n_tab == R.lay["n_tab"] and nbytes == R.lay["payload_off"] + n_t * R.lay["tile_bytes"] <= R.cap
            touched = R.table(r) >= 0
            assert int(touched.sum()) == n_t
            ref_msg = parallel.sparse_pack(R.g[r][r], touched, world, r, h)
            assert torch.equal(R.msg[r][:nbytes], ref_msg), (world, what, r)
            assert nbytes < R.g[r][r].numel() * R.g[r].element_size()
        R.unpack_all()
        R.assert_equals_dense(dense)
        for r in range(world):
            for i in range(len(frames)):
                host = R.fs[r].read_gathered_frame(R.g[r].data_ptr(), i, what)
                if what == abi.EXCHANGE_PLANES:
                    assert np.array_equal(bits(host), bits(refs[i])), (world, r, i)
                else:
                    assert np.array_equal(host, orc.resolve8(tuple(refs[i]))), (world, r, i)
        R.close()


@pytest.mark.parametrize("cfg", [4, 5])
def test_baseline_configs_4_and_5_eight_way_sparse(orc, cfg):
    """BASELINE configs 4 (spot x16, 2048^2) and 5 (8 stacked spots, 4096^2) as specified, 8 ranks, through the sparse exchange"""
    build = {4: scenes.config4, 5: scenes.config5}[cfg]
    frames = [build(3)]
    ref = np.stack(orc.draw(frames[0])[1])
    for what in KINDS:
        R = Ranks(frames, 8, what)
        dense = R.dense().clone()
        R.unpack_all()
        R.assert_equals_dense(dense)
        for r in (0, 5):
            host = R.fs[r].read_gathered_frame(R.g[r].data_ptr(), 0, what)
            if what == abi.EXCHANGE_PLANES:
                assert np.array_equal(bits(host), bits(ref)), (cfg, r)
            else:
                assert np.array_equal(host, orc.resolve8(tuple(ref))), (cfg, r)
        R.close()


# config 2's payload fraction (touched tiles / tiles of the shards), 8 ranks, 1024^2, these four frames: measured 0.165 on MI355X
# (0.001 of the listed tiles all clear); the bound leaves margin
CONFIG2_TOUCHED_MAX = 0.25


def test_touched_set_is_k_clears():
    """the listed tiles are the ones k_clear leaves alone: every tile with a non-clear pixel is listed; a listed tile may be all clear
    (a bounding box reaches it without covering a pixel), but few are"""
    frames = [scenes.config2(i, size=1024) for i in (0, 7, 19, 30)]
    R = Ranks(frames, 8, abi.EXCHANGE_PLANES)
    listed = nonclear = total = 0
    for r in range(8):
        t = R.table(r) >= 0
        nc = parallel.nonclear_tiles(R.g[r][r], r, 8, 1024)
        assert not bool((nc & ~t).any()), r          # a drawn tile that is not sent would be lost
        listed, nonclear, total = listed + int(t.sum()), nonclear + int(nc.sum()), total + t.numel()
    assert (listed - nonclear) <= 0.25 * listed, (listed, nonclear)
    assert listed / total < CONFIG2_TOUCHED_MAX, listed / total
    print(f"config 2, 8 ranks: {listed / total:.3f} of the tiles touched, {(listed - nonclear) / listed:.3f} of them all clear")
    R.close()


def test_frames_without_fused_clear_send_every_tile_and_empty_frames_none():
    """frame 0 is rendered over pre-filled planes without FUSED_CLEAR (its untouched tiles keep the old contents: all of them are
    sent); frame 1 has no triangles and a fused clear (nothing to send); both reassemble exactly"""
    w, h, world = 200, 150, 3
    empty = abi.Frame(w, h, scenes.EYE, scenes.LIGHTS, [], abi.FUSED_CLEAR)
    frames = [spot(4, w, h, flags=0), empty]
    for what in KINDS:
        R = Ranks(frames, world, what, flags=0, prefill=0.25)
        dense = R.dense().clone()
        for r in range(world):
            t = R.table(r) >= 0
            n_local = parallel.shard_layout(h, r, world)["n_local_bands"]
            assert bool(t[0, :n_local].all()) and not bool(t[0, n_local:].any()), r
            assert not bool(t[1].any()), r
        R.unpack_all()
        R.assert_equals_dense(dense)
        R.close()


def test_pack_captures_its_render():
    """render A, pack; then a sceneset update + render changes the tile counts: A's message still unpacks to A"""
    import srz
    from srz import scenes as pscenes
    world, r_src = 2, 0
    wl = pscenes.spot_texture_1024(size=256)
    wl.frame(0)                                   # (registers the texture slots)
    lib = srz.lib()
    lib.srz_sceneset_update.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.SrzSceneFrame), C.c_int]
    ranks = []
    for r in range(world):
        ctx = srz.Context(0, r, world)
        wl.upload_meshes(ctx), wl.upload_textures(ctx)
        fs = ctx.frameset([wl.scene_frame(0), wl.scene_frame(9)])
        ranks.append((ctx, fs))
    ctx, fs = ranks[r_src]
    g = torch.zeros((world,) + fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render(g[r_src].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR)          # (everything on the ctx's own stream)
    cap = fs.sparse_capacity()
    msg = torch.zeros((world, cap), dtype=torch.uint8, device="cuda")
    fs.sparse_pack(g[r_src].data_ptr(), msg[r_src].data_ptr(), cap)
    ctx.sync()
    a_shard, a_msg = g[r_src].clone(), msg[r_src].clone()
    later = [wl.scene_frame(18), wl.scene_frame(27)]
    ctx._check(lib.srz_sceneset_update(ctx.h, fs.h, abi.scene_frames_array(later), 2))
    other = torch.zeros_like(g[r_src])
    fs.render(other.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR)
    ctx.sync()
    assert not torch.equal(other, a_shard)
    assert torch.equal(msg[r_src], a_msg)
    ctx_d, fs_d = ranks[1]
    gd = torch.full((world,) + fs.out_shape, -1.0, dtype=torch.float32, device="cuda")
    fs_d.sparse_unpack(msg.data_ptr(), cap, gd.data_ptr())
    ctx_d.sync()
    real = torch.zeros(fs.local_rows, dtype=torch.bool, device="cuda")
    for (lb, _, r0, r1) in parallel.band_rows(256, r_src, world):
        real[lb * 32: lb * 32 + r1 - r0] = True
    assert torch.equal(gd[r_src][:, :, real].view(torch.int32), a_shard[:, :, real].view(torch.int32))
    for c, f in ranks:
        f.close(), c.close()


def test_world_one_communicator_and_misuse():
    import srz
    ctx = srz.Context(0)
    ctx.texture_upload(0, scenes.spot_texture())
    comm = srz.Comm(ctx, srz.Comm.unique_id(), 0, 1)
    frames = [scenes.config2(i, size=256) for i in (1, 2)]
    fs = ctx.frameset(frames)
    out = torch.zeros(fs.out_shape, dtype=torch.float32, device="cuda")
    fs.render(out.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, 0)
    cap = fs.sparse_capacity()
    assert cap == parallel.sparse_layout(2, 8, 256)["capacity"] and fs.sparse_capacity(7) == 0
    msg = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    fs.sparse_pack(out.data_ptr(), msg.data_ptr(), cap, abi.EXCHANGE_PLANES, 0)
    before = out.clone()
    recv = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    fs.allgather_sparse(comm, msg.data_ptr(), recv.data_ptr(), cap, out.data_ptr(), abi.EXCHANGE_PLANES, 0)   # world 1: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(out, before) and not bool(recv.any())
    for bad in (lambda: fs.sparse_pack(out.data_ptr(), msg.data_ptr(), cap - 16, abi.EXCHANGE_PLANES, 0),
                lambda: fs.sparse_pack(out.data_ptr(), 0, cap, abi.EXCHANGE_PLANES, 0),
                lambda: fs.sparse_pack(out.data_ptr(), msg.data_ptr(), cap, 7, 0),
                lambda: fs.sparse_unpack(0, cap, out.data_ptr()),
                lambda: fs.allgather_sparse(comm, 0, recv.data_ptr(), cap, out.data_ptr()),
                lambda: fs.allgather_sparse(comm, msg.data_ptr(), recv.data_ptr(), cap, 0)):
        with pytest.raises(srz.SrzError) as e:
            bad()
        assert e.value.code == abi.SRZ_E_INVALID
    ctx2 = srz.Context(0, 1, 2)   # a frameset of another shard
    fs2 = ctx2.frameset(frames)
    with pytest.raises(srz.SrzError) as e:
        fs2.allgather_sparse(comm, msg.data_ptr(), recv.data_ptr(), cap, out.data_ptr())
    assert e.value.code == abi.SRZ_E_INVALID
    fs2.close(), ctx2.close()
    comm.close()
    fs.close(), ctx.close()


def _two_rank_worker(rank, world, port, q):
    import conftest  # noqa: F401
    import torch.distributed as dist
    import srz
    from oracle import oracle
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)   # (rendezvous only: the exchange is srz_comm's RCCL)
    try:
        try:
            oracle.texture_set(0, scenes.spot_texture())
            ctx = srz.Context(rank, rank, world)
            ctx.texture_upload(0, scenes.spot_texture())
            ids = [srz.Comm.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            comm = srz.Comm(ctx, ids[0], rank, world)
            frames = [scenes.config2(i, size=256) for i in (3, 8)]
            fs = ctx.frameset(frames)
            g = torch.zeros((world,) + fs.out_shape, dtype=torch.float32, device="cuda")
            st = torch.cuda.Stream()
            fs.render(g[rank].data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, st.cuda_stream)
            cap = fs.sparse_capacity()
            msg = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            fs.sparse_pack(g[rank].data_ptr(), msg.data_ptr(), cap, abi.EXCHANGE_PLANES, st.cuda_stream)
            recv = torch.zeros(world * cap, dtype=torch.uint8, device="cuda")
            fs.allgather_sparse(comm, msg.data_ptr(), recv.data_ptr(), recv.numel(), g.data_ptr(), abi.EXCHANGE_PLANES, st.cuda_stream)
            st.synchronize()
            ok = True
            for i, f in enumerate(frames):
                ref = np.stack(oracle.draw(f)[1])
                ok = ok and np.array_equal(fs.read_gathered_frame(g.data_ptr(), i).view(np.uint32), ref.view(np.uint32))
            # one rank's receive buffer too small: BOTH ranks get SRZ_E_NOMEM (no rank enters the second collective alone)
            short = 64 if rank == 1 else recv.numel()
            code = None
            try:
                fs.allgather_sparse(comm, msg.data_ptr(), recv.data_ptr(), short, g.data_ptr(), abi.EXCHANGE_PLANES, st.cuda_stream)
            except srz.SrzError as e:
                code = e.code
            st.synchronize()
            q.put((rank, ok and code == abi.SRZ_E_NOMEM, code))
            comm.close()
        except BaseException as e:  # noqa: BLE001  (the parent must not wait for a worker that died)
            q.put((rank, f"worker failed: {e!r}", None))
            raise
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")
def test_two_ranks_sparse_allgather_over_rccl():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    procs = [mctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert all(ok is True for _, ok, _ in res), res
