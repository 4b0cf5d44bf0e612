"""What the tests of the vertex stage's backward share (tests/test_vertex_grad_ref.py on the CPU, tests/test_gpu_vertex_grad.py and
tests/test_gpu_scene_fit.py on the device): shared-vertex meshes, perspective matrices whose w varies over a mesh, and a float64
restatement of the vertex stage.  Nothing of the product."""
import types

import numpy as np

import chainref
from support import col_major, place, vertex_stage, xform_div_w


def perspective(sx, sy, ox, oy, w=2.0, wx=0.35, wy=-0.25, wz=0.5, sz=1.5, oz=3.0, shear=0.05):
    """unit coordinates -> pixels with a real divide: r3 = w + wx x + wy y + wz z varies over the mesh, rows 0 .. 2 are (sx x + ox) w,
    (sy y + oy) w and (sz z + oz) w plus a little shear — for a mesh in the unit cube r3 stays within [w - |wy|, w + wx + wz]"""
    return col_major([[sx * w, shear * sx, 0.1 * sx, ox * w], [-shear * sy, sy * w, 0.07 * sy, oy * w],
                      [0.02, -0.03, sz * w, oz * w], [wx, wy, wz, w]])


def verts8(pos):
    """[V, 3] positions -> [V, 8] float32 vertex records, flat normals, uv = the position's (x, y)"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    v = np.zeros((len(pos), 8), np.float32)
    v[:, 0:3], v[:, 5], v[:, 6:8] = pos, -1.0, pos[:, 0:2]
    return v


def oriented(pos, faces, m):
    """the faces with the corner order whose stored screen area under matrix m is negative (the winding that survives the cull for the
    eye at (0, 0, 1)); a face of zero area is kept as it is"""
    xy = xform_div_w(m, np.asarray(pos, np.float32))[:, :2].astype(np.float64)
    f = np.array(faces, np.uint32).reshape(-1, 3)
    a, b, c = xy[f[:, 0]], xy[f[:, 1]], xy[f[:, 2]]
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    f[area > 0] = f[area > 0][:, [0, 2, 1]]
    return f


def grid(nx, ny, seed, extra=0, z=0.5, jitter=0.2):
    """nx x ny vertices over the unit square (jittered inside their cells, depth about z) as 2 (nx - 1)(ny - 1) triangles — an interior
    vertex is shared by six faces — plus `extra` vertices in a row above the square, each tied to the mesh by one more face ->
    (pos [V, 3] float32, faces [F, 3])"""
    rng = np.random.default_rng([seed, 83])
    ys, xs = np.mgrid[0:ny, 0:nx].astype(np.float64)
    cell = np.array([1.0 / (nx - 1), 1.0 / (ny - 1)])
    xy = np.stack([xs.ravel(), ys.ravel()], 1) * cell + rng.uniform(-jitter, jitter, (nx * ny, 2)) * cell
    pos = np.concatenate([xy, z + rng.uniform(-0.1, 0.1, (nx * ny, 1))], 1)
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            faces += [(a, b, d), (b, c, d)] if (i + j) % 2 else [(a, b, c), (a, c, d)]
    for e in range(extra):
        pos = np.concatenate([pos, [[(e + 0.5) * cell[0], -0.6 * cell[1], z]]])
        faces.append((len(pos) - 1, e + 1, e))
    return pos.astype(np.float32), np.array(faces, np.uint32)


def fan(n, seed, z=0.5):
    """a hub (vertex 0) with n faces around it — its corner list is longer than a wave for n > 64 —, one vertex no face names
    (vertex n + 2) and one face (v, v, w) that names vertex 1 twice -> (pos [n + 3, 3], faces [n + 1, 3])"""
    rng = np.random.default_rng([seed, 89])
    ang = np.linspace(0.0, 2 * np.pi, n + 1, endpoint=True) + 0.1
    rad = rng.uniform(0.3, 0.45, n + 1)
    ring = 0.5 + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None]
    pos = np.concatenate([[[0.5, 0.5]], ring, [[0.05, 0.05]]])
    pos = np.concatenate([pos, z + rng.uniform(-0.1, 0.1, (len(pos), 1))], 1)
    faces = [(0, 1 + i, 2 + i) for i in range(n)] + [(1, 1, 3)]
    return pos.astype(np.float32), np.array(faces, np.uint32)


def single():
    """one face, three vertices"""
    return np.float32([[0.15, 0.2, 0.4], [0.85, 0.3, 0.5], [0.4, 0.9, 0.6]]), np.array([[0, 1, 2]], np.uint32)


def stage64(pos, m, zscale, zoffset):
    """the vertex stage restated in float64: pos [V, 3], m 16 floats column-major -> screen positions [V, 3]"""
    m = np.asarray(m, np.float64).reshape(4, 4).T  # rows
    p = np.asarray(pos, np.float64)
    r = p @ m[:, :3].T + m[:, 3]
    return np.stack([r[:, 0] / r[:, 3], r[:, 1] / r[:, 3], r[:, 2] / r[:, 3] * zscale + zoffset], 1)


# ------------------------------------------------------------------------------------------------------ a scene of chainref's kind
def chain_scene(seed):
    """a 48 x 40 scene of chainref's kind whose triangles come out of support.vertex_stage: a 4 x 4-vertex patch (18 faces, interior
    vertices shared six ways) in front of a 3 x 3-vertex patch, both of ONE mesh, under a perspective ndc_mvp; then chainref's backdrop"""
    near, fn = grid(4, 4, seed, z=0.1)
    far, ff = grid(3, 3, seed + 50, z=0.8)
    near[:, :2] = near[:, :2] * 0.55 + [0.05, 0.1]
    far[:, :2] = far[:, :2] * 0.6 + [0.35, 0.3]
    pos = np.concatenate([near, far]).astype(np.float32)
    m = perspective(40.0, 32.0, 4.0, 4.0, w=2.0, wx=0.3, wy=-0.2, wz=0.4, sz=4.0, oz=1.0, shear=0.02)
    faces = oriented(pos, np.concatenate([fn, ff + len(near)]), m)
    return types.SimpleNamespace(pos=pos, faces=faces, m=m, zs=np.float32(1.0), zo=np.float32(0.0))


def chain_positions(s, pos, m):
    """the scene's screen positions [T, 3, 3] float32 out of support.vertex_stage for vertex positions pos and matrix m, the backdrop last"""
    t = vertex_stage(verts8(pos), s.faces, m, np.eye(4, dtype=np.float32).reshape(16), s.zs, s.zo)
    return np.concatenate([t["pos"], chainref.BACKDROP[None]]).astype(np.float32)


def backdrop_mesh():
    """chainref's backdrop as a mesh of its own: under support.place(1, 1, 0, 0) (every row times 2, divided by 2 again) and the depth
    mapping (1, 0) the vertex stage returns its coordinates bit for bit"""
    return np.array(chainref.BACKDROP, np.float32), np.array([[0, 1, 2]], np.uint32)


def abs_jacobians(pos, faces, m, zscale, zoffset):
    """|d screen position / d parameter| of one draw from a float64 restatement (torch on the CPU), for carrying a bound on gpos to a
    bound on the vertex stage's gradients: (|J_verts| [F, 3, 3, V, 3], |J_m| [F, 3, 3, 16], |J_zmap| [F, 3, 3, 2])"""
    import torch
    f = torch.as_tensor(np.asarray(faces, np.int64))

    def stage(v, mm, zm):
        rows = mm.view(4, 4).T
        r = v @ rows[:, :3].T + rows[:, 3]
        return torch.stack([r[:, 0] / r[:, 3], r[:, 1] / r[:, 3], r[:, 2] / r[:, 3] * zm[0] + zm[1]], 1)[f]
    args = (torch.as_tensor(np.asarray(pos, np.float64)), torch.as_tensor(np.asarray(m, np.float64).reshape(16)),
            torch.tensor([float(zscale), float(zoffset)], dtype=torch.float64))
    return tuple(j.abs().numpy() for j in torch.autograd.functional.jacobian(stage, args))


# ------------------------------------------------------------------------------------------------------ fitting a pose and a mesh
# chainref.pose_scene's flat-coloured triangles as a mesh of three vertices of its own per triangle, in pixels, drawn through
# support.place(1, 1, tx, ty, w = FIT_W): its translation entries m[12], m[13] are FIT_W times the offset in pixels.  Two descents of
# chainref.POSE_STEPS steps towards the frame rendered at chainref.POSE_OFFSET, the loss 0.5 * sum (out - target)^2:
#   matrix: on m[12] and m[13], lr = chainref.POSE_LR * FIT_W^2 — chainref's own pose recovery, step for step;
#   verts:  on every vertex's x and y freely, lr = FIT_VERTS_LR; the error is the mean distance of the vertices to where the target
#           has them, 1.000 pixel at the start.  A vertex can slide along an outline the image hardly sees, so this one stalls
#           between 0.27 and 0.43 pixel.
# Measured through the CPU references (tests/test_vertex_grad_ref.py runs the loops again and holds them to these; DESIGN.md has the
# table), per seed of chainref.POSE_SEEDS.  Asserted on the device: below twice the value (matrix: twice the worst, chainref's margin)
FIT_W, FIT_VERTS_LR = 2.0, 0.03
FIT_MATRIX_FINAL = {2: 0.1198, 4: 0.0263, 5: 0.0000, 7: 0.0284}
FIT_VERTS_FINAL = {2: 0.3599, 4: 0.2713, 5: 0.4273, 7: 0.3056}
FIT_MATRIX_BOUND = 2 * max(FIT_MATRIX_FINAL.values())


def fit_model(seed):
    """-> (vertex positions [15, 3] in pixels, faces [5, 3], attr [6, 3, 3] flat colours, the backdrop's last)"""
    P, attr = chainref.pose_scene(seed)
    return P[:-1].reshape(-1, 3).copy(), np.arange(3 * (len(P) - 1), dtype=np.uint32).reshape(-1, 3), attr


def fit_matrix(p):
    """the model's ndc_mvp for translation entries p = (m[12], m[13])"""
    return place(1.0, 1.0, float(p[0]) / FIT_W, float(p[1]) / FIT_W, w=FIT_W)


def fit_descend(kind, grad_of, pos):
    """POSE_STEPS steps of plain descent in float32.  grad_of(pos, p) -> (gverts [V, 3], gdraw [18]) of the loss at vertex positions pos
    and translation entries p.  kind "matrix": p moves; "verts": the vertices' x and y move -> the error after every step"""
    p, v = np.zeros(2, np.float32), np.array(pos, np.float32, copy=True)
    target = np.asarray(pos, np.float32)[:, :2] + np.float32(chainref.POSE_OFFSET)
    err = []
    for _ in range(chainref.POSE_STEPS):
        gv, gd = grad_of(v, p)
        assert np.isfinite(gv).all() and np.isfinite(gd).all()
        if kind == "matrix":
            p = (p - np.float32(chainref.POSE_LR * FIT_W * FIT_W) * np.asarray(gd, np.float32)[12:14]).astype(np.float32)
            err.append(float(np.hypot(*(p.astype(np.float64) / FIT_W - chainref.POSE_OFFSET))))
        else:
            v[:, :2] = (v[:, :2] - np.float32(FIT_VERTS_LR) * np.asarray(gv, np.float32)[:, :2]).astype(np.float32)
            err.append(float(np.linalg.norm(v[:, :2].astype(np.float64) - target, axis=1).mean()))
    return np.array(err)
