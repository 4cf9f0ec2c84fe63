#!/usr/bin/env python3
"""
Writes ``flexmf_explicit_quality.json``: the test RMSE the Torch restatement trainer of
``tests/flexmf_explicit_restatement.py`` reaches on ml-latest-small at the default configuration,
end to end on the CPU in float32, over five training seeds -- the yardstick of the quality check
in ``tests/test_gpu_flexmf_explicit.py`` -- and the RMSE of the ``BiasScorer`` alone on the same
split.

The split is ``quick_measure_model``'s (20 % of the rows of a fifth of the users held out), drawn
from ``SPLIT_SEED``; the RMSE is pooled over every held-out rating.

    python tests/golden/make_flexmf_explicit_quality.py
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

SPLIT_SEED = 20240607
SEEDS = [1, 2, 3, 4, 5]


def make_split(ds):
    from lkpy_amd.splitting import SampleFrac, sample_users

    return sample_users(ds, ds.user_count // 5, SampleFrac(0.2, rng=SPLIT_SEED), rng=SPLIT_SEED)


def bias_rmse(split) -> float:
    from lkpy_amd.basic import BiasScorer

    bias = BiasScorer()
    bias.train(split.train)
    errs = [bias(key.user_id, truth).scores().astype(np.float64) -
            np.asarray(truth.field("rating"), np.float64) for key, truth in split.test]
    return float(np.sqrt(np.mean(np.concatenate(errs) ** 2)))


def main():
    from flexmf_explicit_restatement import predict_rmse, train_explicit_restatement
    from lkpy_amd.data import load_movielens_npz
    from lkpy_amd.flexmf import FlexMFExplicitConfig

    split = make_split(load_movielens_npz(HERE / "ml_small.npz"))
    out = {"split_seed": SPLIT_SEED, "seeds": SEEDS, "test_ratings": split.test_size,
           "bias_rmse": bias_rmse(split), "rmse": []}
    print("bias", out["bias_rmse"], flush=True)
    for seed in SEEDS:
        tabs, g = train_explicit_restatement(split.train, FlexMFExplicitConfig(), seed)
        val = predict_rmse(tabs, g, split.train, split.test)
        print(seed, val, flush=True)
        out["rmse"].append(val)
    (HERE / "flexmf_explicit_quality.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
