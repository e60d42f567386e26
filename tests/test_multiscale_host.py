"""Host side of the multi-resolution network, without a GPU: ``geometry.prefix_levels`` (sizes, offsets and row ids for uniform
and ragged batches, including the ``ceil``), and ``models.DeltaNetMultiscaleSegmentation``'s ``state_dict`` keys and constructor
errors; the existing segmentation model keeps its keys."""
import pytest
import torch

from deltaconv_amd.geometry import prefix_levels
from deltaconv_amd.geometry.graph import PtrInfo


def info_of(sizes, with_min=True):
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    return PtrInfo(ptr, len(sizes), max(sizes), min(sizes) if with_min else None)


def test_prefix_levels_of_a_uniform_batch():
    levels = prefix_levels(info_of([256, 256, 256]), (4, 2))
    assert [l[2][2] for l in levels] == [256, 64, 32] and [l[2].min_cloud for l in levels] == [256, 64, 32]
    assert levels[0][0] is None and levels[0][1].tolist() == [0, 256, 512, 768]
    for (rows, ptr, info), n in zip(levels[1:], (64, 32)):
        assert ptr.dtype == torch.int64 and ptr.tolist() == [0, n, 2 * n, 3 * n]
        assert info[0].dtype == torch.int32 and info[0].tolist() == ptr.tolist() and info[1] == 3
        assert rows.dtype == torch.int64 and rows.tolist() == [b * 256 + i for b in range(3) for i in range(n)]
    # ceil: 10 points by 4 keep 3, those by 2 keep 2
    levels = prefix_levels(info_of([10, 10]), (4, 2))
    assert [l[1].tolist() for l in levels] == [[0, 10, 20], [0, 3, 6], [0, 2, 4]]
    assert levels[1][0].tolist() == [0, 1, 2, 10, 11, 12] and levels[2][0].tolist() == [0, 1, 10, 11]
    assert len(prefix_levels(info_of([7]), ())) == 1


@pytest.mark.parametrize("with_min", (True, False))
def test_prefix_levels_of_a_ragged_batch(with_min):
    sizes = [256, 200, 9]
    levels = prefix_levels(info_of(sizes, with_min), (4, 3))
    want = [sizes, [64, 50, 3], [22, 17, 1]]                                    # ceil(9 / 4) = 3, ceil(50 / 3) = 17, ceil(3 / 3) = 1
    start = [0, 256, 456]
    for (rows, ptr, info), n in zip(levels, want):
        assert ptr.tolist() == [0, n[0], n[0] + n[1], sum(n)] and info[0].tolist() == ptr.tolist()
        assert info[2] == max(n) and info.min_cloud == min(n)
        if rows is not None:
            assert rows.tolist() == [start[b] + i for b in range(3) for i in range(n[b])]
    with pytest.raises(ValueError, match="ratios"):
        prefix_levels(info_of(sizes), (4, 0))


def test_state_dict_keys_and_constructor_errors():
    from deltaconv_amd.models import DeltaNetMultiscaleBase, DeltaNetMultiscaleSegmentation, DeltaNetSegmentation
    model = DeltaNetMultiscaleSegmentation(3, 6, enc_channels=((16, 16), (32,), (32,)), dec_channels=(32, 16), ratios=(4, 2),
                                           num_neighbors=16, k_down=8)
    keys = list(model.state_dict())
    heads = {k.split(".")[0] for k in keys}
    assert heads == {"deltanet_base", "lin_global", "segmentation_head"}
    convs = {".".join(k.split(".")[1:4]) if k.split(".")[1] == "enc" else ".".join(k.split(".")[1:3])
             for k in keys if k.startswith("deltanet_base.")}
    assert convs == {"enc.0.0", "enc.0.1", "enc.1.0", "enc.2.0", "dec.0", "dec.1"}
    base = model.deltanet_base
    assert base.enc[0][0].centralized and not base.enc[0][1].centralized and not base.enc[1][0].centralized
    assert all(c.v_mlp is not None for level in base.enc for c in level)
    assert base.dec[0].v_mlp is None and base.dec[1].v_mlp is not None          # only the last decoder drops the vector stream
    assert (base.dec[1].in_channels, base.dec[1].out_channels) == (32 + 32, 16)
    assert (base.dec[0].in_channels, base.dec[0].out_channels) == (16 + 16, 32)
    assert model.lin_global[0][0].weight.shape[1] == 16 + 16 + 32
    assert DeltaNetMultiscaleSegmentation(3, 6, categorical_vector=True).lin_categorical is not None
    for kw in (dict(ratios=(4,)), dict(dec_channels=(128,)), dict(ratios=(4, 4, 4)), dict(enc_channels=((64,), ()), ratios=(4,),
                                                                                      dec_channels=(64,))):
        with pytest.raises(ValueError, match="levels|layer"):
            DeltaNetMultiscaleBase(3, **kw)
    with pytest.raises(ValueError, match="vector_pool"):
        DeltaNetMultiscaleBase(3, vector_pool="min")
    # the existing model: the keys it had before the head was factored out
    torch.manual_seed(0)
    old = DeltaNetSegmentation(3, 5, conv_channels=[8, 8], embedding_size=32, categorical_vector=True)
    assert [k.split(".")[0] for k in old.state_dict()][0] == "deltanet_base" and "deltanet_base.convs.0.s_mlp.0.0.weight" in old.state_dict()
    assert {k.split(".")[0] for k in old.state_dict()} == {"deltanet_base", "lin_global", "lin_categorical", "segmentation_head"}
