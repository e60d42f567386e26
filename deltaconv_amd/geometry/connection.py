"""Parallel transport between tangent frames on the device (reference: deltaconv/geometry/connection.py).

``build_transport``, ``angle_in_plane`` and ``rotate_around`` keep the reference's names, positional order, defaults and
result shapes; each is one elementwise launch (csrc/connection.hip).  ``build_graph_transport`` is the same connection for
every edge of a fixed-k graph in one launch, without the ``[E,3]`` expansions of the reference's call shape, and
``transport_sum`` aggregates the neighbours' vectors in the centre's frame -- the vector stream's counterpart of the scalar
sum / mean aggregation -- with a backward over the graph's CSC (no atomics, the same bits on every run).

None of the geometry here is differentiable (the reference's versions are, through autograd): an input that requires grad
while grad mode is on raises ``RuntimeError`` instead of cutting the graph silently.  ``transport_sum`` gives the gradient
with respect to ``v`` only.  There is no CPU path."""
import torch

from .._lib import lib, require_gpu
from ._cross import device as _device, no_grad_inputs as _no_grad_inputs, rows3 as _rows3
from .graph import Graph, _GRAPH_OF

__all__ = ["build_transport", "angle_in_plane", "rotate_around", "build_graph_transport", "transport_sum"]


def build_transport(target_n, target_x, target_y, source_n, source_x, non_oriented=True):
    """Per pair m the 2 x 2 matrix (row-major, ``[M,4]``) that takes coordinates in the source frame to the target frame
    (connection.py:6-47).  Normals that point apart are reconciled by a flip; with ``non_oriented`` the result then carries
    the reflection."""
    require_gpu()
    fn = "build_transport"
    _no_grad_inputs(fn, target_n=target_n, target_x=target_x, target_y=target_y, source_n=source_n, source_x=source_x)
    tn = _rows3(fn, "target_n", target_n)
    m = tn.shape[0]
    tx, ty = _rows3(fn, "target_x", target_x, m), _rows3(fn, "target_y", target_y, m)
    sn, sx = _rows3(fn, "source_n", source_n, m), _rows3(fn, "source_x", source_x, m)
    out = torch.empty((m, 4), dtype=torch.float32, device=tn.device)
    lib.call("dc_build_transport", tn, tx, ty, sn, sx, None, 1, m, int(bool(non_oriented)), out)
    return out


def angle_in_plane(u, v, normal):
    """Angle from ``u`` to ``v`` in the plane orthogonal to ``normal`` -> ``[M,1]`` (connection.py:50-59)."""
    require_gpu()
    fn = "angle_in_plane"
    _no_grad_inputs(fn, u=u, v=v, normal=normal)
    u = _rows3(fn, "u", u)
    m = u.shape[0]
    v, normal = _rows3(fn, "v", v, m), _rows3(fn, "normal", normal, m)
    out = torch.empty((m, 1), dtype=torch.float32, device=u.device)
    lib.call("dc_angle_in_plane", u, v, normal, m, out)
    return out


def rotate_around(v, axis, angle):
    """``v`` turned about ``axis`` by ``angle`` (``[M]`` or ``[M,1]``) -> ``[M,3]`` (connection.py:62-76)."""
    require_gpu()
    fn = "rotate_around"
    _no_grad_inputs(fn, v=v, axis=axis, angle=angle)
    v = _rows3(fn, "v", v)
    m = v.shape[0]
    axis = _rows3(fn, "axis", axis, m)
    _device(fn, "angle", angle)
    if angle.numel() != m or angle.dim() > 2 or (angle.dim() == 2 and angle.shape[1] != 1):
        raise ValueError(f"{fn}: angle must be [{m}] or [{m},1], got {tuple(angle.shape)}")
    angle = angle.detach().float().reshape(m).contiguous()
    out = torch.empty((m, 3), dtype=torch.float32, device=v.device)
    lib.call("dc_rotate_around", v, axis, angle, m, out)
    return out


def _graph_of(fn, edge_index, n):
    """Graph | an edge_index handed out by one | any centre-major fixed-k edge_index of n points -> Graph."""
    if isinstance(edge_index, Graph):
        g = edge_index
    else:
        g = _GRAPH_OF.get(id(edge_index))
        if g is None or g._edge_index is not edge_index:
            if not torch.is_tensor(edge_index) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
                raise ValueError(f"{fn}: edge_index must be a Graph or a [2,E] tensor")
            if n == 0 or edge_index.shape[1] % n:
                raise ValueError(f"{fn}: edge_index with {edge_index.shape[1]} edges is no fixed-k graph of {n} points")
            g = Graph.from_edge_index(edge_index, n)
    if g.n != n:
        raise ValueError(f"{fn}: edge_index is a graph of {g.n} points, the other arguments have {n}")
    return g


def build_graph_transport(normal, x_basis, y_basis, edge_index, non_oriented=True):
    """The connection of every edge of a fixed-k graph -> ``[N*k,4]``, edge ``i*k + s`` from the frame of ``nbr[i,s]`` into
    the frame of ``i``: ``build_transport(normal[row], x_basis[row], y_basis[row], normal[col], x_basis[col])`` with
    ``row, col = edge_index`` in one launch and the same bits.  ``edge_index``: a ``Graph``, an ``edge_index`` handed out
    by one, or any centre-major fixed-k ``edge_index``."""
    require_gpu()
    fn = "build_graph_transport"
    _no_grad_inputs(fn, normal=normal, x_basis=x_basis, y_basis=y_basis)
    normal = _rows3(fn, "normal", normal)
    n = normal.shape[0]
    xb, yb = _rows3(fn, "x_basis", x_basis, n), _rows3(fn, "y_basis", y_basis, n)
    g = _graph_of(fn, edge_index, n)
    out = torch.empty((n * g.k, 4), dtype=torch.float32, device=normal.device)
    lib.call("dc_build_transport", normal, xb, yb, normal, xb, g.nbr, g.k, n * g.k, int(bool(non_oriented)), out)
    return out


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


class _TransportSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, coef, graph, scale):
        if v.stride(1) != 1 and v.shape[1] != 1 or _ld(v) < v.shape[1]:
            v = v.contiguous()
        out = torch.empty((v.shape[0], v.shape[1]), dtype=torch.float32, device=v.device)
        lib.call("dc_transport_sum", graph.nbr, graph.n, graph.k, coef, v, v.shape[1], _ld(v), scale, out, _ld(out))
        ctx.coef, ctx.graph, ctx.scale = coef, graph, scale
        return out

    @staticmethod
    def backward(ctx, grad):
        graph = ctx.graph
        tptr, tedge = graph.csc()
        if grad.dtype != torch.float32 or (grad.stride(1) != 1 and grad.shape[1] != 1) or _ld(grad) < grad.shape[1]:
            grad = grad.float().contiguous()
        dv = torch.empty((grad.shape[0], grad.shape[1]), dtype=torch.float32, device=grad.device)
        lib.call("dc_transport_sum_backward", tptr, tedge, graph.n, graph.k, ctx.coef, grad, grad.shape[1], _ld(grad), ctx.scale,
                 dv, _ld(dv), 0)
        return dv, None, None, None


def transport_sum(v, connection, edge_index, weights=None, reduce="sum"):
    """Sum (``reduce`` = ``"sum"`` | ``"add"``) or mean (``"mean"``: 1/k) over the k neighbours of every point of their
    vectors brought into the point's frame: ``out[2i+a] = scale * sum_s sum_b R[i,s,a,b] * v[2 nbr[i,s] + b]``, ``v`` and
    ``out`` ``[2N,C]`` in the layout of ``geometry.operators`` (rows 2i, 2i+1 = the two components at point i),
    ``connection`` ``[N*k,4]`` as ``build_graph_transport`` returns it.  ``weights [N*k]`` are multiplied into the connection
    once (one fp32 rounding) before the launch.  Slots are summed in order, every product and sum rounded on its own; the
    backward (gradient with respect to ``v`` only) walks the graph's CSC in ascending edge order: no atomics, the same bits
    on every run, capturable in a ``torch.cuda.graph`` once the CSC exists.  Pass a ``Graph`` (or an ``edge_index`` handed out
    by one) to keep the CSC between calls."""
    require_gpu()
    fn = "transport_sum"
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"{fn}: reduce must be 'sum', 'add' or 'mean', got {reduce!r}")
    _no_grad_inputs(fn, connection=connection, weights=weights)
    _device(fn, "v", v)
    if v.dim() != 2 or v.shape[0] % 2:
        raise ValueError(f"{fn}: v must be [2N,C] (rows 2i, 2i+1 = the two components at point i), got {tuple(v.shape)}")
    if v.dtype != torch.float32:
        raise TypeError(f"{fn}: v must be float32, got {v.dtype}")
    n = v.shape[0] // 2
    g = _graph_of(fn, edge_index, n)
    e = n * g.k
    if not torch.is_tensor(connection) or not connection.is_cuda or tuple(connection.shape) != (e, 4):
        got = tuple(connection.shape) if torch.is_tensor(connection) else type(connection).__name__
        raise ValueError(f"{fn}: connection must be a device tensor of shape [{e},4] (one matrix per edge), got {got}")
    coef = connection.detach().float().contiguous()
    if weights is not None:
        if not torch.is_tensor(weights) or not weights.is_cuda or weights.numel() != e:
            got = tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__
            raise ValueError(f"{fn}: weights must be a device tensor of {e} entries (one per edge), got {got}")
        coef = weights.detach().float().reshape(e, 1) * coef
    scale = 1.0 / g.k if reduce == "mean" else 1.0
    return _TransportSum.apply(v, coef, g, scale)
