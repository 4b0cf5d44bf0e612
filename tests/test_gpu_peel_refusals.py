"""-m gpu: what srz_frameset_peel_visibility refuses, and in which words.  One call per case: every argument is valid but the one
the case names; the call returns SRZ_E_INVALID, leaves the case's text in srz_last_error and launches nothing — the
sentinel-filled output keeps every word."""
import ctypes as C

import pytest
import torch

import srz
from srz import abi
from support import SENTINEL, filled, frame, soup, stream, words

pytestmark = pytest.mark.gpu

W = H = 64
BYTES = 2 * 4 * H * W * 4  # the two-frame sets' buffer
FN = "srz_frameset_peel_visibility: "
NULL = FN + "null frameset / previous layer / output"
ALIGN = FN + "buffers must be 16-byte aligned"
OVERLAP = FN + "the previous layer and the output overlap"
WRONG_SHARD = "frameset was created under a different shard (call srz_set_shard before srz_frameset_create)"

# (the faulty arguments, the text; None: no ctx to hold one).  ("prev" | "out", offset): that buffer's address plus `offset` bytes
CASES = [
    (dict(ctx=None), None),
    (dict(fs=None), NULL),
    (dict(prev=None), NULL),
    (dict(out=None), NULL),
    (dict(out_bytes=BYTES - 1), FN + "output buffer too small"),
    (dict(out_bytes=0), FN + "output buffer too small"),
    (dict(prev=("prev", 4)), ALIGN),
    (dict(out=("out", 8)), ALIGN),
    (dict(out=("prev", 0)), OVERLAP),          # in place
    (dict(out=("prev", 64)), OVERLAP),
    (dict(prev=("out", BYTES - 16)), OVERLAP),  # the last 16 bytes
    (dict(fs="sharded"), WRONG_SHARD),
]


@pytest.fixture(scope="module")
def kit():
    c, cs = srz.Context(0), srz.Context(0, 0, 2)
    frames = [frame(soup(s, 24, W, H, [1.0, 2.0, 3.0])) for s in (1, 2)]
    fs, fs_sharded = c.frameset(frames), cs.frameset(frames)
    prev = torch.zeros((BYTES + 256) // 4, dtype=torch.int32, device="cuda")
    fs.render_visibility(prev.data_ptr(), fs.out_bytes, abi.FUSED_CLEAR, stream())
    torch.cuda.synchronize()
    yield dict(ctx=c, fs=fs, sharded=fs_sharded, prev=prev, prev_words=words(prev).copy())
    fs.close(), fs_sharded.close(), c.close(), cs.close()


@pytest.mark.parametrize("fault,text", CASES, ids=[",".join(f"{k}={v}" for k, v in f.items()) for f, _ in CASES])
def test_refused_with_a_message_and_nothing_launched(kit, fault, text):
    out = filled(((BYTES + 256) // 4,))
    bufs = dict(prev=kit["prev"], out=out)
    args = dict(ctx=kit["ctx"].h, fs=kit["fs"].h, prev=("prev", 0), out=("out", 0), out_bytes=BYTES)
    args.update(fault)
    if args["fs"] == "sharded":
        args["fs"] = kit["sharded"].h
    ptr = {k: None if args[k] is None else C.c_void_p(bufs[args[k][0]].data_ptr() + args[k][1]) for k in ("prev", "out")}
    rc = srz.lib().srz_frameset_peel_visibility(args["ctx"], args["fs"], ptr["prev"], ptr["out"], args["out_bytes"], abi.FUSED_CLEAR,
                                                srz._stream(stream()))
    assert rc == abi.SRZ_E_INVALID
    if text is not None:
        assert srz.lib().srz_last_error(kit["ctx"].h).decode() == text
    torch.cuda.synchronize()
    assert (words(out) == SENTINEL).all() and (words(kit["prev"]) == kit["prev_words"]).all()
