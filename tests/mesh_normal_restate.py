"""numpy restatement of csrc/mesh_normal_math.h -- the vertex-to-corner lists and the per-vertex normals of a store of meshes, fp32
with every operation rounded on its own and the sum of a vertex SEQUENTIAL over its list in ascending ``3 * face_row + corner``
from +0 -- plus the fp64 evaluation of the same formula with the error bound of the header, and the meshes both test files use
(tests/test_mesh_normal_host.py, tests/test_gpu_mesh_normal.py)."""
import functools

import numpy as np

EPS = 1e-12
U = 2.0 ** -24
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------
SPECS = [dict(n_faces=1), dict(n_faces=2, zero_area=1), dict(n_faces=63), dict(n_faces=300, zero_area=5, shrink=(40, 0.01)),
         dict(n_faces=2051, zero_area=3), dict(n_faces=512)]
NAMES = ["F1", "F2", "F63", "F300", "F2051", "torus512", "fan300"]
TORUS, FAN, HOLES = 5, 6, 3                        # the closed torus, the fan, the mesh with unreferenced vertices and shrunk faces
FAN_FACES = 300


def fan_mesh(n=FAN_FACES):
    """n triangles around hub vertex 0 over a wavy rim: one list of n corners, longer than a wave is wide.
    -> (vert float32 [n+1,3], face int64 [n,3])"""
    th = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(th), np.sin(th), 0.1 * np.sin(3 * th) + 0.05 * np.cos(7 * th)], axis=1)
    vert = np.concatenate([[[0.03, -0.02, 0.3]], rim]).astype(np.float32)
    i = np.arange(n)
    return vert, np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n], axis=1)


@functools.lru_cache(maxsize=None)
def meshes():
    """The seven meshes, in the order of NAMES -> [(vert float32 [V,3], face int64 [F,3], y int64 [V])]."""
    from deltaconv_amd.data import synthetic_mesh
    out = []
    for spec in SPECS:
        pos, face, y = synthetic_mesh(seed=3, labels=True, **spec)
        out.append((pos.numpy(), face.t().contiguous().numpy(), y.numpy()))
    vert, face = fan_mesh()
    out.append((vert, face, np.arange(vert.shape[0], dtype=np.int64) % 8))
    return out


def torus(seed):
    from deltaconv_amd.data import synthetic_mesh
    pos, face, y = synthetic_mesh(512, seed=seed, labels=True)
    return pos.numpy(), face.t().contiguous().numpy(), y.numpy()


def store_arrays(ms):
    """[(vert, face, ...)] -> (vert [Vs,3] f32, face [Fs,3] i32 local ids, vptr [B+1] i64, fptr [B+1] i64) of the concatenated store."""
    vert = np.concatenate([m[0] for m in ms]).astype(np.float32)
    face = np.concatenate([m[1] for m in ms]).astype(np.int32)
    vptr = np.concatenate([[0], np.cumsum([m[0].shape[0] for m in ms])]).astype(np.int64)
    fptr = np.concatenate([[0], np.cumsum([m[1].shape[0] for m in ms])]).astype(np.int64)
    return vert, face, vptr, fptr


# ---- lists ------------------------------------------------------------------------------------------------------------------------------
def lists(face, vptr, fptr, num_verts):
    """-> (vf_ptr int64 [num_verts+1], vf_edge int64 [number of valid corners]): per vertex row its corner slots 3 * face_row + corner,
    ascending.  A face row with an id outside [0, V) of its mesh is in no list."""
    face = np.asarray(face, dtype=np.int64)
    vs, es = [], []
    for b in range(len(vptr) - 1):
        rows = np.arange(fptr[b], fptr[b + 1])
        nv = vptr[b + 1] - vptr[b]
        ids = face[rows]
        ok = ((ids >= 0) & (ids < nv)).all(axis=1)
        vs.append((vptr[b] + ids[ok]).reshape(-1))
        es.append((3 * rows[ok, None] + np.arange(3)[None, :]).reshape(-1))
    v, e = np.concatenate(vs), np.concatenate(es)
    keep = v < num_verts
    v, e = v[keep], e[keep]
    order = np.lexsort((e, v))
    vf_ptr = np.zeros(num_verts + 1, dtype=np.int64)
    vf_ptr[1:] = np.cumsum(np.bincount(v, minlength=num_verts))
    return vf_ptr, e[order].astype(np.int64)


def _mesh_of_face(fptr, rows):
    return np.searchsorted(fptr, rows, side="right") - 1


def _norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def contributions(vert, face, vptr, fptr, weighting, dtype=np.float32):
    """What every face row gives to each of its corners -> [Fs,3] in `dtype`, every operation rounded on its own."""
    vert, face = np.asarray(vert, dtype=np.float32).astype(dtype), np.asarray(face, dtype=np.int64)
    base = np.asarray(vptr)[_mesh_of_face(fptr, np.arange(face.shape[0]))]
    p0, p1, p2 = vert[base + face[:, 0]], vert[base + face[:, 1]], vert[base + face[:, 2]]
    a, b = p1 - p0, p2 - p0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                 axis=1)
    if weighting == "area":
        return c
    assert weighting == "uniform"
    return c / np.maximum(_norm3(c), dtype(EPS))[:, None]


def normals(vert, face, vptr, fptr, weighting="uniform", vf=None):
    """-> (normals float32 [Vs,3], zero_count int64 [B]) with the bits of csrc/mesh_normal_math.h."""
    nv = vert.shape[0]
    vf_ptr, vf_edge = lists(face, vptr, fptr, nv) if vf is None else vf
    t = contributions(vert, face, vptr, fptr, weighting)
    assert t.dtype == np.float32
    length = np.diff(vf_ptr)
    s = np.zeros((nv, 3), dtype=np.float32)
    for k in range(int(length.max()) if nv else 0):                # step k of every list at once: each sum stays sequential
        live = np.flatnonzero(length > k)
        s[live] = s[live] + t[vf_edge[vf_ptr[live] + k] // 3]
    n = s / np.maximum(_norm3(s), f32(EPS))[:, None]
    assert n.dtype == np.float32
    zero = ~n.any(axis=1)
    mesh = np.searchsorted(vptr, np.arange(nv), side="right") - 1
    return n, np.bincount(mesh[zero], minlength=len(vptr) - 1).astype(np.int64)


# ---- fp64 and the bound -------------------------------------------------------------------------------------------------------------------
def expected64(vert, face, vptr, fptr, weighting="uniform"):
    """The same formula in fp64 on the fp32 vertices -> (n64 [Vs,3], bound [Vs], s_is_zero [Vs]): the bound of
    csrc/mesh_normal_math.h, ((8 sum w_f + (L + 4) sum |t_f|) u) / |s64| + 4u, infinite where s64 = 0."""
    nv = vert.shape[0]
    vf_ptr, vf_edge = lists(face, vptr, fptr, nv)
    t = contributions(vert, face, vptr, fptr, weighting, np.float64)
    v64, f = np.asarray(vert, dtype=np.float32).astype(np.float64), np.asarray(face, dtype=np.int64)
    base = np.asarray(vptr)[_mesh_of_face(fptr, np.arange(f.shape[0]))]
    a, b = v64[base + f[:, 1]] - v64[base + f[:, 0]], v64[base + f[:, 2]] - v64[base + f[:, 0]]
    ab, cn = _norm3(a) * _norm3(b), _norm3(np.cross(a, b))
    w = ab if weighting == "area" else np.where(cn > 0, ab / np.where(cn > 0, cn, 1.0), 0.0)
    owner = np.repeat(np.arange(nv), np.diff(vf_ptr))
    fr = vf_edge // 3
    s = np.zeros((nv, 3))
    np.add.at(s, owner, t[fr])
    sum_w = np.bincount(owner, weights=w[fr], minlength=nv)
    sum_t = np.bincount(owner, weights=_norm3(t[fr]), minlength=nv)
    sn = _norm3(s)
    n64 = s / np.maximum(sn, EPS)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(sn > 0, ((8 * sum_w + (np.diff(vf_ptr) + 4) * sum_t) * U) / sn + 4 * U, np.inf)
    return n64, bound, sn == 0
