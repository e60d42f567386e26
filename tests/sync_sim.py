"""Data-parallel ranks of synchronised BatchNorm, simulated in ONE process (no process group, no subprocess).

The protocol of deltaconv_amd/dp.py: each rank writes one fp64 record [sum_0 (C) | sum_1 (C) | rows], the record is summed
over ranks in place (`dp.all_reduce_stats`), everything downstream reads the sum.  One process can play all ranks if it
knows the sums before a rank needs them -- by PROGRESSIVE REPLAY:

    pass p:  fn(rank, shard) runs for every rank.  The i-th collective of a rank is answered from totals[i] when that is
             known (stats.copy_(totals[i])); the FIRST unknown index of the pass is recorded (a clone of the rank's
             record), later unknown ones stay local and their downstream results are thrown away with the pass.
    after :  totals[i] = sum of the ranks' records in rank order (fp64, on the records' device).
    end   :  the first pass that meets no unknown collective; its return values are the result.

`collectives + 1` passes.  What makes this valid is that the code under test is deterministic: a record presented again
in a later pass must equal, bit for bit, what was recorded for that (index, rank) -- asserted at every collective,
together with the records of one index having one length on all ranks.  `fn` must therefore build fresh state in every
call (copy.deepcopy of the module: running statistics and num_batches_tracked move in every pass) and keep dropout off.

Patched while the context is open, restored on exit (also after an exception): `dp.sync_state`, `dp.all_reduce_stats`
(both are looked up through the module at call time, in dp.py and nn/fused.py) and `torch.distributed.get_world_size`
for the simulator's own sentinel group (only `fused.check_bn_rows` asks).
"""
import contextlib

import torch
import torch.distributed as dist

from deltaconv_amd import dp


class SimGroup:
    """Sentinel standing in for a process group of `world` ranks."""

    def __init__(self, world):
        self.world = int(world)

    def __repr__(self):
        return f"SimGroup(world={self.world})"


class SyncSim:
    def __init__(self, world):
        self.group = SimGroup(world)
        self.world = int(world)
        self.on = True              # what dp.sync_state() answers: the group, or None (toggle tests)
        self.totals = []            # totals[i]: the all-reduced record of collective i, once known
        self.recorded = {}          # (i, rank) -> the record that rank presented at collective i (a clone)
        self.passes = 0
        self.rank = None
        self._index = 0
        self._saved = None

    # ---- patching ------------------------------------------------------------------------------------------------------
    def __enter__(self):
        assert self._saved is None, "SyncSim is not re-entrant"
        self._saved = (dp.sync_state, dp.all_reduce_stats, dist.get_world_size)
        real_world_size = dist.get_world_size

        def get_world_size(group=None):
            return group.world if isinstance(group, SimGroup) else real_world_size(group)

        dp.sync_state = lambda: self.group if self.on else None
        dp.all_reduce_stats = self._all_reduce
        dist.get_world_size = get_world_size
        return self

    def __exit__(self, *exc):
        dp.sync_state, dp.all_reduce_stats, dist.get_world_size = self._saved
        self._saved = None
        return False

    # ---- the collective ------------------------------------------------------------------------------------------------
    def _all_reduce(self, stats, group):
        assert group is self.group, f"collective over {group!r}, not the simulated group"
        assert self.rank is not None, "collective outside SyncSim.run"
        assert stats.dtype == torch.float64 and stats.dim() == 1, "a record is a flat fp64 vector"
        i, key = self._index, (self._index, self.rank)
        self._index += 1
        if key in self.recorded:         # seen in an earlier pass: the replay must present the same bits
            assert self.recorded[key].shape == stats.shape and torch.equal(self.recorded[key], stats), \
                f"collective {i} of rank {self.rank} changed between passes: the run is not deterministic"
        if i < len(self.totals):
            assert self.totals[i].shape == stats.shape, f"collective {i}: record length differs from the other ranks'"
            stats.copy_(self.totals[i])
        elif i == len(self.totals):      # the first unknown collective of this pass
            for r in range(self.rank):
                assert self.recorded[(i, r)].shape == stats.shape, f"collective {i}: ranks disagree on the record length"
            self.recorded[key] = stats.detach().clone()
        return stats                     # (later unknown ones: left local, ignored)

    # ---- the driver ----------------------------------------------------------------------------------------------------
    def run(self, fn, shards, max_passes=200):
        """fn(rank, shard) for every rank, pass after pass -> [fn's return value per rank] of the final pass.
        A pass whose unknown collective lay in fn's forward part may skip its backward: `self.pending()` says so."""
        assert self._saved is not None, "use inside `with SyncSim(world) as sim:`"
        assert len(shards) == self.world
        while True:
            assert self.passes < max_passes, "no fixed point: too many collectives"
            self.passes += 1
            counts, out = [], []
            for rank, shard in enumerate(shards):
                self.rank, self._index = rank, 0
                try:
                    out.append(fn(rank, shard))
                finally:
                    self.rank = None
                counts.append(self._index)
            known = len(self.totals)
            if all(c <= known for c in counts):
                assert len(set(counts)) == 1, f"ranks ran different numbers of collectives: {counts}"
                return out
            assert all(c > known for c in counts), f"ranks ran different numbers of collectives: {counts}"
            total = self.recorded[(known, 0)].clone()
            for r in range(1, self.world):
                total += self.recorded[(known, r)]
            self.totals.append(total)

    @contextlib.contextmanager
    def as_rank(self, rank):
        """Code that must NOT reach a collective's answer (a refusal every rank raises on its own): run it as `rank`."""
        self.rank, self._index = rank, 0
        try:
            yield self
        finally:
            self.rank = None

    @property
    def seen(self):
        """Collectives the rank that ran last has presented in its current pass."""
        return self._index

    @property
    def collectives(self):
        return len(self.totals)

    def pending(self):
        """True while the current pass has already met its unknown collective (what follows is thrown away)."""
        return self._index > len(self.totals)
