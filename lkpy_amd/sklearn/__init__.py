"""
Mirror of ``lenskit.sklearn``: the scorers the reference builds on scikit-learn, trained on the
device here -- ``svd.BiasedSVDScorer`` (randomized truncated SVD) and ``nmf.NMFScorer``
(NNDSVDA start, Frobenius coordinate descent).
"""
