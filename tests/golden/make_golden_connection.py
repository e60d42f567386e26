"""Golden vectors for the parallel-transport module: run the REAL reference functions (deltaconv/geometry/connection.py, pure
torch, imported from /root/reference with the stand-ins of tools/ref_shims) on seeded inputs, in fp32 and on the same inputs
widened to fp64.  Build container only.

  a_*  2 048 random pairs of unit normals with build_tangent_basis frames, non_oriented True (T) and False (F)
  b_*  2 048 pairs whose source normal is a 5 % perturbation of the target's (neighbours on a smooth surface)
  c_*  every edge of geom_normals_B2_N128_k20.npz (its normal / x_basis / y_basis _f32 and edge_index are the inputs)
  d_*  1 024 rows each for rotate_around and angle_in_plane, built as the reference's test/geometry/test_connection.py does"""
import os
import sys

import numpy as np
import torch
import torch.linalg as LA

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tools", "ref_shims"), "/root/reference"]
from deltaconv.geometry.connection import angle_in_plane, build_transport, rotate_around   # noqa: E402
from deltaconv.geometry.grad_div_mls import build_tangent_basis                             # noqa: E402

out = {}


def unit(x):
    return x / LA.norm(x, dim=1, keepdim=True).clamp(1e-8)


def both(fn, *args, **kw):
    return fn(*args, **kw).numpy(), fn(*(a.double() for a in args), **kw).numpy()


def pairs(tag, tn, sn, flags):
    tx, ty = build_tangent_basis(tn)
    sx, _ = build_tangent_basis(sn)
    for name, t in (("tn", tn), ("tx", tx), ("ty", ty), ("sn", sn), ("sx", sx)):
        out[f"{tag}_{name}"] = t.numpy()
    for flag in flags:
        o32, o64 = both(build_transport, tn, tx, ty, sn, sx, non_oriented=flag)
        out[f"{tag}_out32_{'T' if flag else 'F'}"], out[f"{tag}_out64_{'T' if flag else 'F'}"] = o32, o64


g = torch.Generator().manual_seed(2024)
pairs("a", unit(torch.randn(2048, 3, generator=g)), unit(torch.randn(2048, 3, generator=g)), (True, False))
tn = unit(torch.randn(2048, 3, generator=g))
pairs("b", tn, unit(tn + 0.05 * torch.randn(2048, 3, generator=g)), (True,))

scene = np.load(os.path.join(HERE, "geom_normals_B2_N128_k20.npz"))
nrm, xb, yb = (torch.from_numpy(scene[f"{n}_f32"]) for n in ("normal", "x_basis", "y_basis"))
row, col = torch.from_numpy(scene["edge_index"])
out["c_out32"], out["c_out64"] = both(build_transport, nrm[row], xb[row], yb[row], nrm[col], xb[col])

# rotate_around: unit v, an orthogonal axis (first 768 rows; the angles 90 / 180 / 360 degrees in turn) or any axis (360 degrees)
n = 1024
v = unit(torch.rand(n, 3, generator=g))
axis, _ = build_tangent_basis(v)
axis[768:] = torch.rand(256, 3, generator=g)
angle = torch.tensor([torch.pi / 2, torch.pi, 2 * torch.pi])[torch.arange(n) % 3]
angle[768:] = 2 * torch.pi
out["d_rot_v"], out["d_rot_axis"], out["d_rot_angle"] = v.numpy(), axis.numpy(), angle.numpy()
out["d_rot_out32"], out["d_rot_out64"] = both(rotate_around, v, axis, angle)

# angle_in_plane: u = e_x and v at a random angle in the xy-plane, both carried into the frame of a random normal
ang = torch.rand(n, 1, generator=g) * torch.pi
u = torch.zeros(n, 3)
u[:, 0] = 1
w = torch.cat([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)], dim=1)
normal = unit(torch.rand(n, 3, generator=g))
fx, fy = build_tangent_basis(normal)
T = torch.stack([fx, fy, normal], dim=2)
u, w = torch.bmm(T, u.unsqueeze(-1)).squeeze(-1), torch.bmm(T, w.unsqueeze(-1)).squeeze(-1)
out["d_ang_u"], out["d_ang_v"], out["d_ang_normal"], out["d_ang_angle"] = u.numpy(), w.numpy(), normal.numpy(), ang.numpy()
out["d_ang_out32"], out["d_ang_out64"] = both(angle_in_plane, u, w, normal)

np.savez_compressed(os.path.join(HERE, "connection.npz"), **out)
print("wrote connection.npz", len(out), os.path.getsize(os.path.join(HERE, "connection.npz")))
