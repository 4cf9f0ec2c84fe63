"""
Mirror of ``lenskit.sklearn``: the scorers the reference builds on scikit-learn, trained on the
device here.  Only the SVD half exists (``svd.BiasedSVDScorer``); NMF is not provided.
"""
