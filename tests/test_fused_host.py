"""Host logic of deltaconv_amd.nn.fused (no GPU, the library is never loaded): `bn_mode`, the one place a pass through a
BatchNorm layer decides batch / running statistics, the momentum and the running buffers, advances num_batches_tracked and
drops the cached inference coefficients -- and the order of validation and side effect in `linear_stats`.
Reference semantics: torch.nn.BatchNorm1d.forward (the reference's nn/mlp.py:10, nn/nonlin.py:24-35 run through it)."""
import pytest
import torch

from deltaconv_amd.nn import fused

EPS = 1e-5      # BatchNorm1d's default

# (training, track_running_stats, momentum) -> (use_batch_stats, momentum handed to the kernels, running buffers handed over,
#                                              increment of num_batches_tracked)
# momentum None: the cumulative average 1 / num_batches_tracked, read AFTER the increment (first call: 1 / 1); without
# tracking no buffers exist, so even eval() normalises with batch statistics and no momentum is consumed (0.0)
TABLE = {
    (True, True, 0.1): (True, 0.1, True, 1),
    (True, True, None): (True, 1.0, True, 1),
    (True, False, 0.1): (True, 0.1, False, 0),
    (True, False, None): (True, 0.0, False, 0),
    (False, True, 0.1): (False, 0.1, True, 0),
    (False, True, None): (False, 0.0, True, 0),
    (False, False, 0.1): (True, 0.1, False, 0),
    (False, False, None): (True, 0.0, False, 0),
}


def _bn(training=True, track=True, momentum=0.1):
    return torch.nn.BatchNorm1d(8, momentum=momentum, track_running_stats=track).train(training)


@pytest.mark.parametrize("training,track,momentum", sorted(TABLE, key=str))
def test_bn_mode_table(training, track, momentum):
    use_batch, mom, buffers, bump = TABLE[(training, track, momentum)]
    bn = _bn(training, track, momentum)
    got = fused.bn_mode(bn, rows=4)
    assert len(got) == 5
    assert got[0] is use_batch
    assert type(got[1]) is float and got[1] == mom
    if buffers:
        assert got[2] is bn.running_mean and got[3] is bn.running_var
    else:
        assert got[2] is None and got[3] is None
    assert type(got[4]) is float and got[4] == EPS
    if track:
        assert int(bn.num_batches_tracked) == bump
        fused.bn_mode(bn)                                       # (without a row check as well)
        assert int(bn.num_batches_tracked) == 2 * bump
    else:
        assert bn.num_batches_tracked is None


def test_bn_mode_defers_the_counter_with_a_fixed_momentum():
    bn = _bn()
    with fused.defer_counters():
        assert fused.bn_mode(bn, 4)[1] == 0.1 and fused.bn_mode(bn, 4)[1] == 0.1
        assert int(bn.num_batches_tracked) == 0
    assert int(bn.num_batches_tracked) == 2


def test_bn_mode_cumulative_average_increments_at_once():
    bn = _bn(momentum=None)
    with fused.defer_counters():                            # the momentum is read off the counter: nothing to defer
        assert fused.bn_mode(bn, 4)[1] == 1.0 / 1
        assert int(bn.num_batches_tracked) == 1
        assert fused.bn_mode(bn, 4)[1] == 1.0 / 2
        assert int(bn.num_batches_tracked) == 2
    assert int(bn.num_batches_tracked) == 2


def test_bn_mode_drops_cached_inference_coefficients_in_training_only():
    bn = _bn(training=False)
    bn.running_mean._dc_eval_coeffs = ("key", None)
    fused.bn_mode(bn, 4)
    assert bn.running_mean._dc_eval_coeffs == ("key", None)     # eval: the running statistics do not move
    fused.bn_mode(bn.train(), 4)
    assert not hasattr(bn.running_mean, "_dc_eval_coeffs")


def test_bn_mode_refuses_one_training_row_before_any_side_effect():
    bn = _bn()
    bn.running_mean._dc_eval_coeffs = ("key", None)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        fused.bn_mode(bn, rows=1)
    assert int(bn.num_batches_tracked) == 0 and hasattr(bn.running_mean, "_dc_eval_coeffs")
    assert fused.bn_mode(bn.eval(), rows=1)[0] is False          # inference on one row is fine


def test_linear_stats_validates_before_it_touches_the_layer():
    bn = _bn()
    bn.running_mean._dc_eval_coeffs = ("key", None)
    x, w = torch.randn(4, 8), torch.randn(8, 8)
    with pytest.raises(TypeError, match="linear_stats"):
        fused.linear_stats(x, w, bn, bn.weight, bn.bias)
    assert int(bn.num_batches_tracked) == 0 and hasattr(bn.running_mean, "_dc_eval_coeffs")
