"Graph-based recommendation models -- mirror of ``lenskit.graphs``."
