"""time per epoch of n2v_umap_epoch at n = 1e5 (real cosine neighbours) and 1e6 (random neighbour lists), dim 128,
n_neighbors 15, 5 negatives; device events around runs of epochs, minimum of 5 runs after a warm-up"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from node2vec_amd import umap  # noqa: E402

a, b = umap.find_ab()
for n, real in ((100000, True), (1000000, False)):
    gen = torch.Generator(device="cuda").manual_seed(n)
    if real:
        X = torch.randn((n, 128), generator=gen, device="cuda")
        X = X / X.norm(dim=1, keepdim=True)
        t0 = time.time()
        g = umap.fuzzy_graph(X, 15)
        torch.cuda.synchronize()
        t_graph = time.time() - t0
    else:
        idx = torch.randint(0, n, (n, 15), generator=gen, device="cuda")
        dist = torch.sort(torch.rand((n, 15), generator=gen, device="cuda", dtype=torch.float64) * 0.2 + 0.7, dim=1).values
        t0 = time.time()
        g = umap.fuzzy_graph(None, neighbours=(idx, dist))
        torch.cuda.synchronize()
        t_graph = time.time() - t0
    eps = umap.epochs_per_sample(g.val)
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    Y = [(torch.rand((n, 2), generator=gen, device="cuda") * 20 - 10).contiguous(), torch.empty((n, 2), device="cuda")]
    fired = [int(((torch.floor((e + 1) / eps) > torch.floor(e / eps)) & torch.isfinite(eps)).sum()) for e in (0, 1, 50)]
    def run(k, e0):
        at = 0
        for e in range(e0, e0 + k):
            umap.epoch(g.rowptr, g.col, eps, Y[at], Y[1 - at], e, a, b, 1.0, 1.0 - e / 200.0, 5, 0)
            at = 1 - at
    run(10, 0)
    torch.cuda.synchronize()
    best = 1e9
    for r in range(5):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run(20, 10)
        t.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(t) / 20.0)
    rec = dict(n=n, real_neighbours=real, nnz=int(g.col.numel()), max_degree=int(deg.max()), mean_degree=float(deg.float().mean()),
               rows_over_128=int((deg > 128).sum()), fired_epoch_0_1_50=fired, graph_s=t_graph, ms_per_epoch=best)
    print(json.dumps(rec), flush=True)
