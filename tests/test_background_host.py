"""not-gpu: the background pass's three entry points are declared, exported and bound, their argument tables agree with the header's
prototypes, without a context they refuse; and view_rays, the ray block of a camera, against numpy's binary64 inverse and against the
projection it inverts."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "srz.h")).read()
ENTRY_POINTS = ("srz_frameset_background", "srz_frameset_background_work_bytes", "srz_frameset_background_grad")


def test_header_declares_the_entry_points_under_the_same_abi_version():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int\s+srz_frameset_background\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*const float\s*\*d_ray,\s*"
                     r"uint32_t ray_frames,\s*const float\s*\*d_tex,\s*uint32_t n,\s*uint32_t n_ch,\s*uint32_t tex_frames,\s*uint32_t where,\s*"
                     r"void\s*\*d_out,\s*size_t out_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert re.search(r"size_t\s+srz_frameset_background_work_bytes\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs\)", code)
    assert re.search(r"int\s+srz_frameset_background_grad\s*\(srz_ctx\s*\*ctx,\s*srz_frameset\s*\*fs,\s*const void\s*\*d_vis,\s*"
                     r"const float\s*\*d_ray,\s*uint32_t ray_frames,\s*const void\s*\*d_gout,\s*const float\s*\*d_tex,\s*uint32_t n,\s*"
                     r"uint32_t n_ch,\s*uint32_t tex_frames,\s*uint32_t where,\s*float\s*\*d_gtex,\s*float\s*\*d_gray,\s*void\s*\*d_work,\s*"
                     r"size_t work_bytes,\s*uint32_t flags,\s*void\s*\*stream\)", code)
    assert "#define SRZ_ABI_VERSION 7" in HEADER
    assert "(additive, same version) the environment behind a visibility buffer, by view ray" in HEADER
    assert re.search(r"#define SRZ_BG_NOBODY 0u", HEADER) and re.search(r"#define SRZ_BG_ALL 1u", HEADER)
    for words in ("INTEGER CORNER", "d_c = fmaf((float)y, ry_c, fmaf((float)x, rx_c, r0_c))", "LEFT UNTOUCHED", "WRITTEN, not added into"):
        assert words in HEADER, words


def test_binding_and_library_export_them():
    import srz
    from srz import abi, visibility
    lib = ctypes.CDLL(srz.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in srz.EXPORTS and hasattr(lib, name)
    for method in ("background", "background_grad", "background_work_bytes"):
        assert callable(getattr(srz.FrameSet, method))
    assert (abi.BG_NOBODY, abi.BG_ALL) == (0, 1)
    assert callable(visibility.background) and callable(visibility.background_grad) and callable(visibility.view_rays)
    assert issubclass(visibility._Background, __import__("torch").autograd.Function)


def test_argument_tables_match_the_prototypes():
    import srz
    from srz import abi
    L = srz.lib()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    tables = (abi.BACKGROUND_ARGTYPES, abi.BACKGROUND_WORK_BYTES_ARGTYPES, abi.BACKGROUND_GRAD_ARGTYPES)
    for name, table in zip(ENTRY_POINTS, tables):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == table == list(getattr(L, name).argtypes), name
    assert [len(t) for t in tables] == [14, 2, 17] and L.srz_frameset_background_work_bytes.restype is ctypes.c_size_t


def test_without_a_context_they_refuse():
    import srz
    L = srz.lib()
    assert L.srz_frameset_background(None, None, None, None, 1, None, 4, 3, 1, 0, None, 0, 0, None) == srz.abi.SRZ_E_INVALID
    assert L.srz_frameset_background_work_bytes(None, None) == 0
    assert L.srz_frameset_background_grad(None, None, None, None, 1, None, None, 4, 3, 1, 0, None, None, None, 0, 0, None) == srz.abi.SRZ_E_INVALID


def test_wrapper_argument_checks_need_no_device():
    import torch
    from srz import visibility

    class FS:
        n_frames = 2

        def interpolate_shape(self, c):
            return (2, c, 8, 8)
    with pytest.raises(ValueError):
        visibility.background_grad(FS(), None, None, None, None, want_gtex=False, want_gray=False)
    with pytest.raises(ValueError):
        visibility._background_args(FS(), None, torch.zeros(6, 4, 4, 3, device="meta"), torch.zeros(1, 9, device="meta"), "some")
    for bad in (torch.zeros(4, 3), torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError):
            visibility.view_rays(bad)
    with pytest.raises(ValueError):
        visibility.view_rays(torch.eye(4), front=0)


# ------------------------------------------------------------------------------------------------------ view_rays
from backgroundref import look_at_lh, perspective_lh_no, screen  # noqa: E402


def cameras():
    """the reference's camera (srz.scenes: eye (0, 0, 0.9) at the origin, 45 handed to a radians api, 0.1 .. 100) and two others → [(S
    [4, 4] float64 in mathematical layout, eye, center, w, h)].  The others have a general up vector: an entry of the inverse that is 0 in exact
    arithmetic is rounding noise in binary64, which no two inversions share to a float32 ulp of itself; the reference's camera has
    such entries too, but its matrices are sparse enough that both inversions give them as exact zeros"""
    out = []
    for eye, center, up, fovy, w, h in (((0, 0, 0.9), (0, 0, 0), (0, 1, 0), 45.0, 1024, 1024), ((1.5, -0.7, 2.0), (0.2, 0.1, -0.3), (0.05, 1, 0.02), 0.9, 640, 360),
                                        ((-3, 4, 1), (0, 0, 0), (0.1, 0.2, 1), 1.3, 100, 70)):
        eye, center, up = np.float64(eye), np.float64(center), np.float64(up)
        out.append((screen(w, h) @ perspective_lh_no(fovy, w / h, 0.1, 100.0) @ look_at_lh(eye, center, up), eye, center, w, h))
    return out


def test_view_rays_is_the_binary64_inverse_rounded_once():
    import torch
    from srz.visibility import view_rays
    S = np.stack([c[0] for c in cameras()])
    got = view_rays(torch.as_tensor(S)).numpy()
    assert got.shape == (3, 9) and got.dtype == np.float32
    for i in range(3):
        inv = np.linalg.inv(S[i][[0, 1, 3], :3])
        want = np.concatenate([inv[:, 2], inv[:, 0], inv[:, 1]])
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got[i].astype(np.float64) - want) <= ulp).all(), i
        one = view_rays(torch.as_tensor(S[i])).numpy()
        assert one.shape == (1, 9) and np.array_equal(one[0], got[i])
        assert np.array_equal(view_rays(torch.as_tensor(S[i]), front=-1).numpy()[0], -got[i])
    # float32 matrices are widened first; the block is differentiable
    S32 = torch.as_tensor(S[1], dtype=torch.float32).requires_grad_()
    r = view_rays(S32)
    r.sum().backward()
    assert r.dtype == torch.float32 and S32.grad is not None and bool(S32.grad.abs().sum() > 0)


def test_a_point_in_front_of_the_eye_lies_on_the_ray_of_its_pixel():
    """in binary64: P in front of the eye projects by S to (x, y); the ray r0 + x rx + y ry (default front: the reference's sign) is
    parallel to P - eye and points the same way"""
    import torch
    from srz.visibility import view_rays
    rng = np.random.default_rng(11)
    for S, eye, center, w, h in cameras():
        block = view_rays(torch.as_tensor(S), dtype=torch.float64).numpy()[0]
        r0, rx, ry = block[0:3], block[3:6], block[6:9]
        fwd = (center - eye) / np.linalg.norm(center - eye)
        side, n = np.cross(fwd, [0.3, 0.5, 0.8]), 0
        side /= np.linalg.norm(side)
        up = np.cross(fwd, side)
        for _ in range(300):  # the eye plus a step towards the centre of view, and sideways
            P = eye + rng.uniform(0.5, 20) * (fwd + 0.3 * rng.uniform(-1, 1) * side + 0.3 * rng.uniform(-1, 1) * up)
            q = S @ np.append(P, 1.0)
            assert q[3] > 0  # in front: the reference's w is the view-space depth
            x, y = q[0] / q[3], q[1] / q[3]
            a, b = r0 + x * rx + y * ry, P - eye
            assert np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b)) <= 1e-9 and a @ b > 0
            n += 0 <= x < w and 0 <= y < h
        assert n >= 100  # (points on the screen among them)


def test_the_reference_cameras_w_is_positive_in_front():
    """the default front = +1 is the reference's convention: the host layer's own matrices (lookAtLH, perspectiveLH_NO) give w > 0
    for the scene's centre, which every workload of srz.scenes looks at"""
    from srz import host
    sc = host.Scene("bg_sign", (0.0, 0.0, 0.9), (0, 0, 0), (0, 1, 0), 64, 64)
    sc.set_view((0.0, 0.0, 0.9), (0, 0, 0), (0, 1, 0))
    sc.set_projection(45.0, 0.1, 100.0)
    v, p, _ = sc.matrices()
    m = p.reshape(4, 4).T.astype(np.float64) @ v.reshape(4, 4).T.astype(np.float64)  # column-major floats -> mathematical layout
    assert (m @ np.float64([0, 0, 0, 1]))[3] > 0 and (m @ np.float64([0, 0, 5.0, 1]))[3] < 0
    sc.close()
