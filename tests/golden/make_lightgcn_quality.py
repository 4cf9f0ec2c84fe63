#!/usr/bin/env python3
"""
Writes ``lightgcn_quality.json``: the NDCG the Torch restatement trainer of
``tests/lightgcn_restatement.py`` reaches on ml-latest-small, end to end on the CPU, for the two
losses at the configuration's defaults over five training seeds -- the yardstick of the quality
check in ``tests/test_gpu_lightgcn.py``.

The protocol is ``make_flexmf_quality.py``'s (``quick_measure_model``'s split drawn from the
same ``SPLIT_SEED``, 20 unseen items per test user, NDCG with the ideal taken over the whole test
row).  If the five runs of a loss spread so far that their floor (lowest minus range) is below
the sanity floor of 0.01, ``epochs`` is raised -- doubled -- until it is not, and the value used is
recorded under ``config``.

    python tests/golden/make_lightgcn_quality.py
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

from make_flexmf_quality import SEEDS, SPLIT_SEED, ndcg_host  # noqa: E402

LOSSES = ["pairwise", "logistic"]
SANITY_FLOOR = 0.01


def main():
    from lightgcn_restatement import train_restatement
    from lkpy_amd.data import load_movielens_npz
    from lkpy_amd.graphs.lightgcn import LightGCNConfig
    from lkpy_amd.splitting import SampleFrac, sample_users

    ds = load_movielens_npz(HERE / "ml_small.npz")
    split = sample_users(ds, ds.user_count // 5, SampleFrac(0.2, rng=SPLIT_SEED), rng=SPLIT_SEED)
    out = {"split_seed": SPLIT_SEED, "seeds": SEEDS, "list_length": 20, "config": {}, "ndcg": {}}
    for loss in LOSSES:
        epochs = LightGCNConfig().epochs
        while True:
            cfg = LightGCNConfig(loss=loss, epochs=epochs)
            vals = []
            for seed in SEEDS:
                items, users = train_restatement(split.train, cfg, seed)
                val = ndcg_host({"u_embed.weight": users, "i_embed.weight": items}, split)
                print(loss, epochs, seed, val, flush=True)
                vals.append(val)
            if min(vals) - (max(vals) - min(vals)) >= SANITY_FLOOR:
                break
            epochs *= 2
        out["config"][loss] = {"epochs": epochs}
        out["ndcg"][loss] = vals
    (HERE / "lightgcn_quality.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
