"""Correctly rounded state checksums (tests/golden/probes.py: state_checksum) of the REAL reference models at the
seed-1 init of the model fixtures made by make_golden.py, for the bitwise same-init check of
tests/test_oracle_golden.py.  The float64 sums stored inside those fixtures come from torch's reduction, whose
order (and so whose last bits) depends on the host.  Runs only in the build container:

    python tests/golden/make_golden_checksums.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tools", "ref_shims"), "/root/reference", ROOT]

from deltaconv.models import DeltaNetClassification, DeltaNetSegmentation   # noqa: E402  (the reference)
from tests.golden.probes import state_checksum                             # noqa: E402

# name -> (kind, k, grad_regularizer, model kwargs): the model_case calls of make_golden.py
CASES = {
    "model_cls_B4_N256_k20": ("cls", 20, 1e-3, dict(in_channels=3, num_classes=40)),
    "model_seg_B2_N256_k20": ("seg", 20, 1e-3, dict(in_channels=3, num_classes=50, categorical_vector=True)),
    "model_cls_nonormals_B2_N256_k20": ("cls", 20, 1e-2, dict(in_channels=3, num_classes=15, conv_channels=[64, 64, 64, 128])),
    "model_seg_depth1_B2_N1024_k30": ("seg", 30, 1e-3, dict(in_channels=3, num_classes=8, conv_channels=[32] * 4, mlp_depth=1,
                                                            embedding_size=128)),
}

if __name__ == "__main__":
    out = {}
    for name, (kind, k, lam, kw) in CASES.items():
        torch.manual_seed(1)                                  # train_*.py --seed 1 default init
        cls = DeltaNetSegmentation if kind == "seg" else DeltaNetClassification
        out[name] = [float(v) for v in state_checksum(cls(num_neighbors=k, grad_regularizer=lam, **kw))]
    path = os.path.join(HERE, "state_checksums.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {path}")
