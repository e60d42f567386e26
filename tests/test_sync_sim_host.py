"""The rank simulator of tests/sync_sim.py on the CPU: the device-agnostic `dp.SyncBatchNorm1d` (the readable statement of
the synchronised-BatchNorm protocol) under simulated, UNEVEN ranks against torch.nn.BatchNorm1d on the concatenated rows,
all in fp64 -- and the two properties the simulator's validity rests on (determinism check, restoration of patched names)."""
import copy

import pytest
import torch
import torch.distributed as dist

from deltaconv_amd import dp
from tests.sync_sim import SyncSim

TOL = 1e-12


def _net():
    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7, bias=False), torch.nn.BatchNorm1d(7), torch.nn.LeakyReLU(0.2),
                              torch.nn.Linear(7, 4, bias=False), torch.nn.BatchNorm1d(4)).double().train()
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.BatchNorm1d):
                g = torch.linspace(0.4, 1.6, m.num_features, dtype=torch.float64)
                g[::3] *= -1
                m.weight.copy_(g)
                m.bias.copy_(torch.linspace(-0.3, 0.3, m.num_features, dtype=torch.float64))
                m.running_mean.copy_(torch.linspace(-1, 1, m.num_features, dtype=torch.float64))
                m.running_var.copy_(torch.linspace(0.5, 2, m.num_features, dtype=torch.float64))
    return net


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= TOL * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("rows", [(1, 6, 13), (1, 1)])
def test_sync_batchnorm_uneven_shards_equal_full_batch(rows):
    ref = _net()
    sync = dp.convert_sync_batchnorm(copy.deepcopy(ref))
    gen = torch.Generator().manual_seed(5)
    total = sum(rows)
    x = torch.randn(total, 5, dtype=torch.float64, generator=gen) * 1.5 + 0.3
    w = torch.randn(total, 4, dtype=torch.float64, generator=gen)
    xs, ws = x.split(rows), w.split(rows)

    def fn(rank, shard):
        net = copy.deepcopy(sync)                  # fresh parameters (.grad = None) and buffers in every pass
        xr = shard.clone().requires_grad_(True)
        y = net(xr)
        (y * ws[rank]).sum().backward()
        return y.detach(), xr.grad, [p.grad for p in net.parameters()], [b.clone() for b in net.buffers()]

    with SyncSim(len(rows)) as sim:
        out = sim.run(fn, xs)
    assert sim.collectives == 4 and sim.passes == 5        # two BatchNorm layers, forward and backward

    xf = x.clone().requires_grad_(True)
    yf = ref(xf)
    (yf * w).sum().backward()
    _close(torch.cat([o[0] for o in out]), yf.detach(), "output")
    _close(torch.cat([o[1] for o in out]), xf.grad, "dx")
    for i, p in enumerate(ref.parameters()):
        _close(sum(o[2][i] for o in out), p.grad, f"parameter gradient {i} (sum over ranks)")
    for i, b in enumerate(ref.buffers()):                  # running mean / variance (unbiased by the GLOBAL count), counter
        for r, o in enumerate(out):
            if b.dtype.is_floating_point:
                _close(o[3][i], b, f"buffer {i} of rank {r}")
            else:
                assert int(o[3][i]) == int(b) == 1, f"num_batches_tracked of rank {r}"
            assert torch.equal(o[3][i], out[0][3][i]), f"buffer {i}: rank {r} differs from rank 0"


def test_determinism_check_fires():
    """A record that changes between passes invalidates the replay: the simulator must say so."""
    sync = dp.convert_sync_batchnorm(_net())
    xs = torch.randn(6, 5, dtype=torch.float64).split((2, 4))

    def fn(rank, shard):
        return copy.deepcopy(sync)(shard + torch.rand(shard.shape, dtype=torch.float64))

    with SyncSim(2) as sim:
        with pytest.raises(AssertionError, match="not deterministic"):
            sim.run(fn, xs)


def test_ranks_must_agree_on_record_length():
    bn4, bn3 = dp.SyncBatchNorm1d(4).double().train(), dp.SyncBatchNorm1d(3).double().train()

    def fn(rank, shard):
        return (bn4, bn3)[rank](shard)

    with SyncSim(2) as sim:
        with pytest.raises(AssertionError, match="record length"):
            sim.run(fn, [torch.randn(3, 4, dtype=torch.float64), torch.randn(3, 3, dtype=torch.float64)])


def test_single_row_decision_under_simulated_ranks():
    """fused.check_bn_rows (host-side, no kernel): a rank with ONE row passes when the statistics span several ranks, a rank
    WITHOUT rows is refused (a global batch of one row leaves every other rank there), one rank in all is refused as before."""
    from deltaconv_amd.nn import fused
    bn = torch.nn.BatchNorm1d(4).train()
    with SyncSim(3):
        fused.check_bn_rows(bn, 1)
        fused.check_bn_rows(bn, 2)
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            fused.check_bn_rows(bn, 0)
    with SyncSim(1):
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            fused.check_bn_rows(bn, 1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        fused.check_bn_rows(bn, 1)
    fused.check_bn_rows(bn.eval(), 1)


def test_patched_names_are_restored():
    before = (dp.sync_state, dp.all_reduce_stats, dist.get_world_size)
    with SyncSim(3) as sim:
        assert dp.sync_state() is sim.group and dist.get_world_size(sim.group) == 3
        sim.on = False
        assert dp.sync_state() is None
    assert (dp.sync_state, dp.all_reduce_stats, dist.get_world_size) == before
    with pytest.raises(KeyError):
        with SyncSim(2):
            raise KeyError("inside")
    assert (dp.sync_state, dp.all_reduce_stats, dist.get_world_size) == before
    assert dp.sync_state() is None
