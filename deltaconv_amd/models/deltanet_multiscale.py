"""A multi-resolution DeltaNet: a U-shaped backbone over a hierarchy of prefix levels (``geometry.prefix_levels``), and its
segmentation model.  The reference ships single-resolution models only and points at this one ("GeodesicFPS is used in the
multiscale architecture", experiments/train_shapenet.py:32); the transitions are this package's: scalars go down by
``CloudPair.down`` (max over the k_down nearest fine points) and up by ``CloudPair.up`` (knn_interpolate), vectors down by
``CloudPair.down_vectors(reduce=vector_pool)`` (parallel transport, then the vector of largest norm) and up by
``CloudPair.up_vectors``.

Level l + 1 keeps the first ``ceil(n / ratios[l])`` rows of every cloud of level l, with their positions, normals and frames: no
sampling runs inside the step.  The hierarchy is a farthest-point-sampling hierarchy exactly when the rows of every cloud are in
FPS pick order, which is where ``geodesic_subsample`` (the dataset recipes) puts them.  That is ``sampling="prefix"``, the default.
With ``sampling="fps"`` one Euclidean farthest-point sampling launch (``geometry.fps_levels``) picks level 1 inside the step and the
deeper levels are prefixes of its picks: a farthest-point hierarchy on rows in any order."""
import torch

from .deltanet_base import _ptr_info
from .deltanet_segmentation import DeltaNetSegmentation
from ..geometry.fps import FPS_METHODS
from ..geometry.graph import Graph, _min_cloud
from ..geometry.grad_div_mls import build_grad_div, build_tangent_basis, estimate_basis
from ..geometry.resample import CloudPair, fps_levels, prefix_levels
from ..nn import DeltaConv

_VECTOR_POOLS = ("interpolate", "max", "mean", "sum", "add")
_SAMPLINGS = ("prefix", "fps")


class DeltaNetMultiscaleBase(torch.nn.Module):
    """``enc_channels[l]``: the widths of the DeltaConv layers of level l on the way down; ``dec_channels[l]``: the width of the
    one DeltaConv that joins level l's encoder output with what comes up from level l + 1; ``ratios[l]``: level l + 1 keeps every
    cloud's first ``ceil(n / ratios[l])`` rows.  ``forward(data)`` -> the list of level-0 scalar features: every output of the
    level-0 encoder, then the output of the level-0 decoder.  ``sampling``: ``"prefix"`` (the default) takes the rows as they
    stand -- a farthest-point hierarchy when they are in FPS pick order; ``"fps"`` runs one Euclidean farthest-point sampling
    launch per forward pass (``geometry.fps_levels``) and is that hierarchy whatever the order of the rows.  ``fps_method``: the
    sampler of ``sampling="fps"``, "brute" | "grid" as in ``geometry.fps`` (None: its switch, ``DC_FPS``); the same hierarchy
    either way, "grid" takes clouds above 16 384 points."""

    def __init__(self, in_channels, enc_channels=((64, 64), (128,), (256,)), dec_channels=(128, 128), ratios=(4, 4), mlp_depth=1,
                 num_neighbors=20, k_down=16, k_up=3, grad_regularizer=0.001, grad_kernel_width=1, vector_pool="max",
                 centralize_first=True, sampling="prefix", fps_method=None):
        super().__init__()
        enc_channels = [list(c) for c in enc_channels]
        levels = len(enc_channels)
        if levels < 1 or any(len(c) < 1 for c in enc_channels):
            raise ValueError("DeltaNetMultiscaleBase: enc_channels needs at least one level and one layer per level")
        if len(ratios) != levels - 1 or len(dec_channels) != levels - 1:
            raise ValueError(f"DeltaNetMultiscaleBase: {levels} levels need {levels - 1} ratios and dec_channels, got "
                             f"{len(ratios)} and {len(dec_channels)}")
        if vector_pool not in _VECTOR_POOLS:
            raise ValueError(f"DeltaNetMultiscaleBase: vector_pool must be one of {_VECTOR_POOLS}, got {vector_pool!r}")
        if sampling not in _SAMPLINGS:
            raise ValueError(f"DeltaNetMultiscaleBase: sampling must be one of {_SAMPLINGS}, got {sampling!r}")
        if fps_method is not None and fps_method not in FPS_METHODS:
            raise ValueError(f"DeltaNetMultiscaleBase: fps_method must be None or one of {FPS_METHODS}, got {fps_method!r}")
        self.sampling, self.fps_method = sampling, fps_method
        self.k, self.k_down, self.k_up = int(num_neighbors), int(k_down), int(k_up)
        self.ratios = [int(r) for r in ratios]
        self.grad_regularizer, self.grad_kernel_width, self.vector_pool = grad_regularizer, grad_kernel_width, vector_pool
        self.enc = torch.nn.ModuleList()
        width = in_channels
        for l, channels in enumerate(enc_channels):
            convs = torch.nn.ModuleList()
            for i, c in enumerate(channels):
                convs.append(DeltaConv(width, c, depth=mlp_depth, centralized=(centralize_first and l == 0 and i == 0), vector=True))
                width = c
            self.enc.append(convs)
        dec, c_up = {}, enc_channels[-1][-1]       # c_up: the channel count coming up
        for l in range(levels - 2, -1, -1):
            dec[l] = DeltaConv(enc_channels[l][-1] + c_up, dec_channels[l], depth=mlp_depth, vector=(l != 0))
            c_up = dec_channels[l]
        self.dec = torch.nn.ModuleList([dec[l] for l in range(levels - 1)])
        self.out_widths = list(enc_channels[0]) + ([dec_channels[0]] if levels > 1 else [])

    def check_levels(self, data):
        """-> the batch's PtrInfo; ``ValueError`` naming the first level whose smallest cloud has fewer than ``num_neighbors``
        points: the host knows ``ceil(min / ratio)``, nothing is launched."""
        info = _ptr_info(data)
        mn = _min_cloud(info)
        for l, r in enumerate([1] + self.ratios):
            mn = -(-mn // r)
            if mn < self.k:
                raise ValueError(f"DeltaNetMultiscale: level {l} has a cloud of {mn} points, fewer than num_neighbors = {self.k}")
        return info

    @torch.no_grad()
    def build_levels(self, data, info=None):
        """-> per level ``(pos, frames, ptr int64, info, graph, grad, div)``, and the ``CloudPair`` between consecutive levels.
        Geometry only: no autograd.  ``info``: what ``check_levels(data)`` returned (called here otherwise)."""
        info = self.check_levels(data) if info is None else info
        pos = data.pos.contiguous().float()
        if getattr(data, "norm", None) is not None:
            normal = data.norm.contiguous().float()
            frames = (normal,) + tuple(build_tangent_basis(normal))
        else:
            frames = tuple(estimate_basis(pos, Graph.knn(pos, 10, ptr_info=info), orientation=pos))
        levels = []
        for rows, ptr, linfo in (fps_levels(pos, info, self.ratios, method=self.fps_method) if self.sampling == "fps" else
                                 prefix_levels(info, self.ratios)):
            p = pos if rows is None else pos[rows]
            fr = frames if rows is None else tuple(t[rows] for t in frames)
            graph = Graph.knn(p, self.k, ptr_info=linfo)
            grad, div = build_grad_div(p, fr[0], fr[1], fr[2], graph, kernel_width=self.grad_kernel_width,
                                       regularizer=self.grad_regularizer)
            levels.append((p, fr, ptr, linfo, graph, grad, div))
        pairs = [CloudPair(f[0], c[0], f[2], c[2], self.k_down, self.k_up, f[1], c[1], differentiable=True,
                           max_fine_cloud=f[3][2], max_coarse_cloud=c[3][2]) for f, c in zip(levels[:-1], levels[1:])]
        return levels, pairs

    def forward(self, data):
        from ..nn import fused
        info = self.check_levels(data)      # before anything is launched
        fused.presplit_begin()      # bf16 planes of every weight the products have asked for: one launch per forward pass
        levels, pairs = self.build_levels(data, info)
        return self._forward_layers(data, levels, pairs)

    def _forward_layers(self, data, levels, pairs):
        x = data.x if getattr(data, "x", None) is not None else data.pos
        v = levels[0][5] @ x
        out, skips = [], []
        for l, convs in enumerate(self.enc):
            graph, grad, div = levels[l][4:7]
            for conv in convs:
                x, v = conv(x, v, grad, div, graph)
                if l == 0:
                    out.append(x)
            if l + 1 < len(self.enc):
                skips.append((x, v))
                x, v = pairs[l].down(x, "max"), pairs[l].down_vectors(v, reduce=self.vector_pool)
        for l in range(len(self.enc) - 2, -1, -1):
            graph, grad, div = levels[l][4:7]
            xs, vs = skips[l]
            x = torch.cat([xs, pairs[l].up(x)], dim=1)
            v = torch.cat([vs, pairs[l].up_vectors(v)], dim=1)
            x, v = self.dec[l](x, v, grad, div, graph)
        if len(self.enc) > 1:
            out.append(x)
        return out


class DeltaNetMultiscaleSegmentation(DeltaNetSegmentation):
    """The head of ``DeltaNetSegmentation`` over the level-0 features of ``DeltaNetMultiscaleBase``."""

    def __init__(self, in_channels, num_classes, enc_channels=((64, 64), (128,), (256,)), dec_channels=(128, 128), ratios=(4, 4),
                 mlp_depth=1, num_neighbors=20, k_down=16, k_up=3, grad_regularizer=0.001, grad_kernel_width=1, vector_pool="max",
                 centralize_first=True, embedding_size=1024, categorical_vector=False, sampling="prefix", fps_method=None):
        super().__init__(in_channels, num_classes, embedding_size=embedding_size, categorical_vector=categorical_vector,
                         backbone=DeltaNetMultiscaleBase(in_channels, enc_channels, dec_channels, ratios, mlp_depth, num_neighbors,
                                                         k_down, k_up, grad_regularizer, grad_kernel_width, vector_pool,
                                                         centralize_first, sampling=sampling, fps_method=fps_method))
