"""not-gpu: the product's C++ host layer (libsrz_host.so: Scene / ObjLoader / TextureLoader / vertex stage) against
the oracle's restatements — bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes as oscenes  # tests/scenes.py: oracle-built inputs
from srz import abi, host
from srz import scenes as pscenes
from support import bits, compile_cpp_program

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_decoder_matches_pil():
    from oracle import objload
    mine = host.load_image_bgr(pscenes.SPOT_TEX)
    ref = objload.load_texture_bgr(pscenes.SPOT_TEX)
    assert mine.shape == (1024, 1024, 3) and np.array_equal(mine, ref)


def test_png_decoder_variants(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    cases = {"rgb": Image.fromarray(rgb), "rgba": Image.fromarray(np.dstack([rgb, rgb[:, :, :1]])),
             "gray": Image.fromarray(rgb[:, :, 0]), "pal": Image.fromarray(rgb).quantize(16)}
    for name, im in cases.items():
        p = str(tmp_path / f"{name}.png")
        im.save(p)
        expect = np.asarray(Image.open(p).convert("RGB"), np.uint8)[:, :, ::-1]
        assert np.array_equal(host.load_image_bgr(p), expect), name
    with pytest.raises(RuntimeError):
        host.load_image_bgr(str(tmp_path / "missing.png"))


def test_png_decoder_rejects_malformed_headers(tmp_path):
    """a palette image that claims 16 bits per sample (no such PNG layout: it used to divide by zero) and absurd sizes must
    raise the loader's error, not crash the host process"""
    import struct
    import zlib

    def png(w, h, depth, ctype, payload=b"\0" * 64):
        def chunk(t, d):
            return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
        return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
                chunk(b"PLTE", bytes(range(48))) + chunk(b"IDAT", zlib.compress(payload)) + chunk(b"IEND", b""))
    for name, data in {"pal16": png(4, 4, 16, 3), "huge": png(1 << 30, 1 << 30, 8, 2), "rgb4": png(4, 4, 4, 2),
                       "toolarge": png(40000, 2, 8, 0)}.items():
        p = tmp_path / f"{name}.png"
        p.write_bytes(data)
        with pytest.raises(RuntimeError):
            host.load_image_bgr(str(p))


def test_jpeg_decoder_against_libjpeg_turbo_fixtures():
    """cv::imread reads JPEG through libjpeg(-turbo) with default settings; the C++ decoder (jpeg_decode.cpp: T.81 baseline +
    progressive, libjpeg's ISLOW inverse DCT, fancy upsampling and colour tables) must return the same bytes.  Expected pixels:
    tests/golden/jpeg/expected.npz, made by tests/golden/make_jpeg_golden.py with Pillow (libjpeg-turbo) in this image — for ten
    small synthetic files and for the height map the reference ships for BUMP / DISPLACEMENT (assets/models/spot/hmap.jpg:
    800 x 800, progressive, 4:2:0)."""
    import zlib
    gold = os.path.join(REPO, "tests", "golden", "jpeg")
    exp = np.load(os.path.join(gold, "expected.npz"))
    names = [n for n in exp.files if not n.startswith("hmap_")]
    assert len(names) == 10
    for n in names:
        got = host.load_image_bgr(os.path.join(gold, n + ".jpg"))
        assert got.shape == exp[n].shape and np.array_equal(got, exp[n]), n
    hm = host.load_image_bgr(os.path.join(REPO, "assets", "models", "spot", "hmap.jpg"))
    assert list(hm.shape) == exp["hmap_shape"].tolist() == [800, 800, 3]
    assert zlib.crc32(hm.tobytes()) == int(exp["hmap_crc32"][0])
    assert np.array_equal(hm[384:416, 384:416], exp["hmap_centre"])
    assert np.array_equal(hm.reshape(-1, 3)[exp["hmap_idx"]], exp["hmap_samples"])


def test_jpeg_decoder_live_against_pillow(tmp_path):
    """the same comparison on files written now (sizes down to 1 x 1, every subsampling, optimised tables, restart markers)"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    for (w, h) in ((1, 1), (2, 5), (17, 13), (64, 48), (250, 3)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[:, : w // 2] = (np.arange(h)[:, None, None] * 255 // max(h - 1, 1)).astype(np.uint8)   # half smooth, half noise
        for mode, subs in (("RGB", (0, 1, 2)), ("L", (None,))):
            for sub in subs:
                for prog in (False, True):
                    for extra in ({}, {"optimize": True, "quality": 35}, {"restart_marker_blocks": 2, "quality": 97}):
                        p = str(tmp_path / f"j{n}.jpg")
                        kw = dict(format="JPEG", progressive=prog, **extra)
                        if sub is not None:
                            kw["subsampling"] = sub
                        Image.fromarray(a if mode == "RGB" else a[:, :, 0], mode).save(p, **kw)
                        expect = np.asarray(Image.open(p).convert("RGB"), np.uint8)[:, :, ::-1]
                        assert np.array_equal(host.load_image_bgr(p), expect), (w, h, mode, sub, prog, extra)
                        n += 1
    assert n == 120


def test_jpeg_decoder_rejects_what_it_does_not_decode(tmp_path):
    """truncated files, a frame header of an unsupported process (arithmetic coding, 12-bit, CMYK), garbage after SOI and corrupt
    tables raise the loader's error (an empty cv::Mat in the reference → its runtime_error), they do not crash the host process
    (the sanitizer side of this is tests/test_host_fuzz.py: seeded mutations of the fixtures through an AddressSanitizer + UBSan build)"""
    good = open(os.path.join(REPO, "tests", "golden", "jpeg", "base_444_64.jpg"), "rb").read()
    sof = good.index(b"\xff\xc0")
    cases = {"no_frame": good[:sof], "arith": good[:sof] + b"\xff\xc9" + good[sof + 2:], "bits12": good[:sof + 4] + b"\x0c" + good[sof + 5:],
             "cmyk": good[:sof + 9] + b"\x04" + good[sof + 10:], "soi_only": b"\xff\xd8\xff", "truncated_seg": good[:sof + 6]}
    for name, data in cases.items():
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        with pytest.raises(RuntimeError):
            host.load_image_bgr(str(p))
    # a Huffman table with more codes of one length than a prefix code has room for (it used to overrun the decoder's look-up table)
    dht = good.index(b"\xff\xc4")
    bad_dht = bytearray(good)
    bad_dht[dht + 5] = 200                       # 200 codes of length 1
    p = tmp_path / "bad_dht.jpg"
    p.write_bytes(bytes(bad_dht))
    with pytest.raises(RuntimeError):
        host.load_image_bgr(str(p))
    # a file cut inside its entropy-coded data still decodes (libjpeg pads with zeros and warns): same size, top rows intact
    cut = tmp_path / "cut.jpg"
    cut.write_bytes(good[:len(good) * 2 // 3])
    a, b = host.load_image_bgr(str(cut)), host.load_image_bgr(os.path.join(REPO, "tests", "golden", "jpeg", "base_444_64.jpg"))
    assert a.shape == b.shape and np.array_equal(a[:16], b[:16])


@pytest.mark.parametrize("path", [pscenes.SPOT_OBJ, pscenes.BUNNY_OBJ])
def test_obj_loader_matches_the_restatement(path):
    v_ref, f_ref = oscenes.mesh(path)
    sc = host.Scene("t", (0, 0, 0.9), (0, 0, 0), (0, 1, 0), 64, 64)
    sc.add_obj(path, "m")
    v, f = sc.mesh("m")
    assert v.shape == v_ref.shape and f.shape == f_ref.shape
    assert np.array_equal(f, f_ref) and np.array_equal(bits(v), bits(v_ref))


def test_obj_loader_quads_negative_indices_and_missing_normals(tmp_path):
    p = tmp_path / "q.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\nf -4/-4 -3/-3 -2/-2\n")
    from oracle import objload
    v_ref, _, f_ref = objload.load_obj(str(p))
    sc = host.Scene("t", (0, 0, 1), (0, 0, 0), (0, 1, 0), 64, 64)
    sc.add_obj(str(p), "q")
    v, f = sc.mesh("q")
    assert len(f) == 3 and np.array_equal(f, f_ref)          # quad fan-triangulated + one triangle
    assert np.array_equal(bits(v), bits(v_ref))
    assert np.allclose(v[:, 7], 1.0 - np.array([0, 0, 1, 1]))  # v -> 1 - v
    assert np.allclose(np.abs(v[:, 5]), 1.0)                   # synthesised normals are +-z


def test_matrices_match_the_oracle(orc):
    W, H = 1920, 1080
    sc = host.Scene("t", (0.1, 0.2, 0.9), (0, 0.1, 0), (0, 1, 0), W, H)
    sc.add_obj(pscenes.SPOT_OBJ, "spot", (0, 1, 0), 0.0, (0, 0, 0), (1, 1, 1))
    sc.set_model("spot", (1, 2, 3), 37.0, (0.3, -0.2, 0.5), (0.3, 0.4, 0.5))
    sc.set_view((0.1, 0.2, 0.9), (0, 0.1, 0), (0, 1, 0))
    sc.set_projection(45.0, 0.1, 100.0)
    v, p, n = sc.matrices()
    assert np.array_equal(bits(v), bits(orc.look_at_lh((0.1, 0.2, 0.9), (0, 0.1, 0), (0, 1, 0))))
    assert np.array_equal(bits(p), bits(orc.perspective_lh_no(45.0, np.float32(W) / np.float32(H), 0.1, 100.0)))
    assert np.array_equal(bits(n), bits(orc.ndc_matrix(W, H)))
    assert np.array_equal(bits(sc.model("spot")), bits(orc.model_matrix((1, 2, 3), 37.0, (0.3, -0.2, 0.5), (0.3, 0.4, 0.5))))


@pytest.mark.parametrize("frame_idx", [0, 7, 23])
def test_vertex_stage_matches_the_oracle_config2(frame_idx):
    wl = pscenes.spot_texture_1024()
    f, fo = wl.frame(frame_idx), oscenes.config2(frame_idx)
    assert len(f.tris) == 1 and np.array_equal(bits(f.tris[0]), bits(fo.tris[0]))
    assert np.array_equal(f.lights, fo.lights)
    assert tuple(f.c.ka) == tuple(fo.c.ka) and f.c.p == 150.0 and tuple(f.c.eye) == tuple(fo.c.eye)
    assert np.array_equal(wl.texture_arrays[0], oscenes.spot_texture())


def test_vertex_stage_matches_the_oracle_config3_and_4():
    for wl, fo in ((pscenes.spot_bunny_1080p(), oscenes.config3(5)), (pscenes.spot_grid16_2048(), oscenes.config4(5))):
        f = wl.frame(5)
        assert len(f.tris) == len(fo.tris)
        for a, b in zip(f.tris, fo.tris):
            assert np.array_equal(bits(a), bits(b))
        assert [int(b.shader) for b in f._batches[:len(f.tris)]] == [int(b.shader) for b in fo._batches[:len(fo.tris)]]


def test_readme_scene_spot_and_crate_matches_the_oracle_side():
    """the README benchmark scene through the C++ ObjLoader (Crate1.obj: quads, fan triangulation, v → 1 - v) and PNG decoder
    vs the oracle-side restatement, bit for bit; and facts any OBJ reader must agree on, taken from the files themselves"""
    wl = pscenes.readme_spot_crate_1024()
    for i in (0, 9):
        f, fo = wl.frame(i), oscenes.readme_scene(i)
        assert [len(t) for t in f.tris] == [5856, 12]
        for a, b in zip(f.tris, fo.tris):
            assert np.array_equal(bits(a), bits(b))
        assert tuple(f.c.eye) == tuple(fo.c.eye) and f.c.eye[2] < 0
    assert np.array_equal(wl.texture_arrays[0], oscenes.spot_texture()) and np.array_equal(wl.texture_arrays[1], oscenes.crate_texture())
    from PIL import Image
    assert np.array_equal(wl.texture_arrays[1], np.asarray(Image.open(pscenes.CRATE_TEX).convert("RGB"), np.uint8)[:, :, ::-1])
    # independent of every loader in this repository: a line-level reading of the file
    for path, mesh_name in ((pscenes.CRATE_OBJ, "Crate"), (pscenes.SPOT_OBJ, "spot")):
        pos, polys = [], []
        for line in open(path):
            w = line.split()
            if w[:1] == ["v"]:
                pos.append([float(x) for x in w[1:4]])
            elif w[:1] == ["f"]:
                polys.append([int(t.split("/")[0]) - 1 for t in w[1:]])
        pos = np.asarray(pos, np.float32)
        v, faces = wl.scene.mesh(mesh_name)                         # (nV, 8) pos3 nrm3 uv2 ; (nF, 3)
        assert len(faces) == sum(len(p) - 2 for p in polys)         # an n-gon makes n - 2 triangles
        file_pos = {tuple(p) for p in pos.tolist()}
        assert {tuple(p) for p in v[:, :3].tolist()} <= file_pos    # no invented positions
        k = 0
        for p in polys:                                             # fan order: (p0, p_i, p_i+1)
            for i in range(1, len(p) - 1):
                tri = v[faces[k], :3]
                assert np.array_equal(tri, pos[[p[0], p[i], p[i + 1]]]), (mesh_name, k)
                k += 1


def test_scene_error_conventions(tmp_path, capfd):
    sc = host.Scene("t", (0, 0, 1), (0, 0, 0), (0, 1, 0), 64, 64)
    sc.add_obj(pscenes.BUNNY_OBJ, "b")
    with pytest.raises(RuntimeError):
        sc.add_obj(pscenes.BUNNY_OBJ, "b")              # duplicate name → false + log
    with pytest.raises(RuntimeError):
        sc.add_obj(str(tmp_path / "nope.obj"), "x")     # unreadable file → false + log
    with pytest.raises(RuntimeError):
        sc.add_shader("s", str(tmp_path / "nope.png"), abi.SHADER_NORMAL)  # every Shader needs a loadable image
    with pytest.raises(RuntimeError):
        sc.bind("b", "missing")
    with pytest.raises(RuntimeError):
        sc.set_model("missing", (0, 1, 0), 0, (0, 0, 0), (1, 1, 1))
    err = capfd.readouterr().err
    assert "already been identified" in err and "Add Shader Failed" in err


def test_lights_documented_intent_and_reference_exact_switch():
    wl = pscenes.spot_texture_1024()
    L = wl.scene.lights()
    assert L.shape == (2, 6) and tuple(L[0]) == (np.float32(0.9), np.float32(0.9), np.float32(-0.9), 100, 100, 100)
    host.lib().srzh_set_reference_exact_lights(wl.scene.h, 1)   # src/Scene.cpp:296-312 as written: default lights
    assert np.array_equal(wl.scene.lights(), np.zeros((2, 6), np.float32))


def test_cpp_api_compiles_like_the_readme_and_refuses_to_run_without_a_gpu(tmp_path):
    """User code written against the reference's README (README.md:127-205) compiles against our headers unchanged."""
    exe = tmp_path / "api_demo"
    cmd = ["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests", "cpp", "api_demo.cpp"), "-I",
           os.path.join(REPO, "software-rasterizer_amd", "host", "include"), "-L", os.path.join(REPO, "software-rasterizer_amd"),
           "-lsrz_host", "-lsrz", f"-Wl,-rpath,{os.path.join(REPO, 'software-rasterizer_amd')}", "-o", str(exe)]
    subprocess.check_call(cmd)
    import torch
    r = subprocess.run([str(exe), REPO], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr   # constructor throws std::runtime_error


def test_target_pipeline_program_compiles_and_refuses_to_run_without_a_gpu(tmp_path):
    """tests/cpp/target_pipeline.cpp (the C++ pipeline over the device-resident target; run by tests/test_gpu_cpp_api.py) builds
    against the headers as they are, and without a device its first constructor throws: exit 3, nothing dumped"""
    exe = compile_cpp_program("target_pipeline", tmp_path)
    import torch
    r = subprocess.run([exe, REPO, str(tmp_path / "dump_")], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, (r.stdout, r.stderr)
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)
        assert not list(tmp_path.glob("dump_*"))


def test_bmp_loader_equals_pillow(tmp_path):
    """cv::imread also reads BMP (src/TextureLoader.cpp:3-12): uncompressed 24-bit, 32-bit (alpha dropped) and 8-bit palettised files,
    odd widths (row padding), against Pillow's decode; RLE and 4-bit files are refused with the loader's error"""
    from PIL import Image
    rng = np.random.default_rng(11)
    for (w, h) in ((1, 1), (5, 3), (17, 13), (64, 2)):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for name, im in (("rgb", Image.fromarray(a[:, :, :3])), ("rgba", Image.fromarray(a)), ("pal", Image.fromarray(a[:, :, :3]).quantize(37)),
                         ("grey", Image.fromarray(a[:, :, 0]))):
            p = str(tmp_path / f"{name}_{w}x{h}.bmp")
            im.save(p)
            expect = np.asarray(Image.open(p).convert("RGB"), np.uint8)[:, :, ::-1]
            assert np.array_equal(host.load_image_bgr(p), expect), (name, w, h)
    good = open(str(tmp_path / "rgb_17x13.bmp"), "rb").read()
    for name, data in (("rle", good[:30] + b"\x01" + good[31:]), ("bpp4", good[:28] + b"\x04" + good[29:]), ("short", good[:100]),
                       ("huge", good[:18] + b"\xff\xff\xff\x7f" + good[22:])):
        q = tmp_path / f"bad_{name}.bmp"
        q.write_bytes(data)
        with pytest.raises(RuntimeError):
            host.load_image_bgr(str(q))
