"""Drives sgns.DeltaSync over `world` replicas held by ONE process, on CPU or device tensors, so that its
result can be laid beside tests/exchange_restatement.py: the stand-in for torch.distributed only moves
bytes, every addition is made by the code under test (shard._rank_ordered_reduce: n2v_delta_reduce on
device tensors, its host form on CPU tensors).

Not a test module: shared by tests/test_exchange_host.py (CPU tensors) and tests/test_exchange_edges_gpu.py.
"""
import numpy as np
import torch

import exchange_restatement as R

WORLDS = (1, 2, 3, 5, 6, 7, 8)


def bf16_tensor(bits, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16).to(device)


def bf16_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def f32_tensor(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).copy()).to(device)


def f32_array(t):
    return t.detach().cpu().contiguous().numpy().copy()


class Ranks:
    """torch.distributed as rank `rank` of `world` sees it inside shard.ordered_sum.  contrib[r][call] is what
    rank r puts on the wire at the call-th exchanged block.  all_to_all_single hands this rank shard `rank` of
    every rank's (zero-padded) buffer, in rank order; all_gather_into_tensor returns this rank's summed shard
    and -- the other ranks' work -- the other shards summed by the same _rank_ordered_reduce.
    between(call) runs while the collective is "in flight": after pack, before apply."""

    def __init__(self, world, rank, contrib, between=None):
        self.world, self.rank, self.contrib, self.between = world, rank, contrib, between
        self.calls = 0
        self.ReduceOp = torch.distributed.ReduceOp

    def get_world_size(self, group=None):
        return self.world

    def get_backend(self, group=None):
        return "stand-in"

    def all_to_all_single(self, recv, send, group=None):
        call, w = self.calls, self.world
        self.calls += 1
        dtype = self.contrib[0][call].dtype
        m = send.numel() // w // self.contrib[0][call].element_size()
        full = torch.zeros(w, w * m, dtype=dtype, device=send.device)
        for r in range(w):
            if r == self.rank:
                full[r].copy_(send.view(dtype))
            else:
                c = self.contrib[r][call].to(send.device)
                full[r, :c.numel()].copy_(c)
        recv.view(dtype).view(w, m).copy_(full[:, self.rank * m:(self.rank + 1) * m])
        self._full, self._m, self._dtype = full, m, dtype
        if self.between is not None:
            self.between(call)

    def all_gather_into_tensor(self, out, shard, group=None):
        from node2vec_amd.shard import _rank_ordered_reduce

        w, m, dtype = self.world, self._m, self._dtype
        rows = out.view(dtype).view(w, m)
        for k in range(w):
            if k == self.rank:
                rows[k].copy_(shard.view(dtype))
                continue
            parts = self._full[:, k * m:(k + 1) * m].contiguous().view(-1)
            rows[k].copy_(_rank_ordered_reduce(parts, w, m, torch.empty(m, dtype=dtype, device=out.device)))


def blocks_of(shapes, block_rows):
    return [(k, lo, min(sh[0], lo + block_rows)) for k, sh in enumerate(shapes)
            for lo in range(0, sh[0], block_rows)]


def run_exchange(device, wire, replicas, refs, block_rows, exact, meanwhile=None, ranks=None):
    """One DeltaSync._exchange per rank in `ranks` (default: all) on `device`.  Arguments as in
    exchange_restatement.exchange (numpy); -> {rank: (matrices, references or None)} as numpy."""
    from node2vec_amd.sgns import DeltaSync

    world = len(replicas)
    shapes = [m.shape for m in replicas[0]]
    blocks = blocks_of(shapes, block_rows)
    syncs = []
    for r in range(world):
        s = DeltaSync([f32_tensor(m, device) for m in replicas[r]], wire=wire, block_rows=block_rows, overlap=False)
        s.active, s.world = True, world
        s.rehearse = world == 1  # a sum of one still goes through the collectives and the reduce pass
        if wire == "bf16":
            s.refs = [bf16_tensor(m, device) for m in refs[r]]
        syncs.append(s)
    contrib = []
    for s in syncs:  # what every rank puts on the wire, block by block, in the order _exchange walks them
        mine = []
        for k, lo, hi in blocks:
            t = s.tensors[k]
            _, w = s._buffers(t)
            n = t[lo:hi].numel()
            s._pack(t[lo:hi], None if s.refs is None else s.refs[k][lo:hi], None, w[:n])
            mine.append(w[:n].clone())
        contrib.append(mine)
    out = {}
    for r in (range(world) if ranks is None else ranks):
        s = syncs[r]
        between = None
        if meanwhile is not None:
            mids = [f32_tensor(m, device) for m in meanwhile[r]]

            def between(call, s=s, mids=mids):
                k, lo, hi = blocks[call]
                s.tensors[k][lo:hi].copy_(mids[k][lo:hi])  # trained on while the sum was on the links

        s.dist = Ranks(world, r, contrib, between)
        s._exchange(exact=exact)
        if device != "cpu":
            torch.cuda.synchronize()
        assert s.dist.calls == len(blocks) and s.exchanged_blocks == len(blocks)
        out[r] = ([f32_array(t) for t in s.tensors], None if s.refs is None else [bf16_bits(t) for t in s.refs])
    return out


def random_case(world, shapes, seed):
    """replicas trained apart from a shared state: well-scaled values, deltas of 1 %"""
    rng = np.random.default_rng(seed)
    base = [rng.standard_normal(sh).astype(np.float32) for sh in shapes]
    replicas = [[b + (0.01 * rng.standard_normal(b.shape)).astype(np.float32) for b in base] for _ in range(world)]
    refs = [[R.ref_init(b) for b in base] for _ in range(world)]
    mids = [[m + (0.01 * rng.standard_normal(m.shape)).astype(np.float32) for m in rep] for rep in replicas]
    return replicas, refs, mids


def special_case(world):
    """the special values of exchange_restatement.edge_case as one column matrix per rank"""
    curs, ref, mids = R.edge_case(world)
    return ([[c.reshape(-1, 1)] for c in curs], [[ref.reshape(-1, 1).copy()] for _ in range(world)],
            [[m.reshape(-1, 1)] for m in mids])


def check_exchange(device, world, wire, case, block_rows, exact, ranks=None):
    """DeltaSync on `device` against the restatement, matrices and references of every checked rank, bit for bit
    -> (elements that differ, what DeltaSync left, what the restatement wants)"""
    replicas, refs, mids = case
    refs = refs if wire == "bf16" else None
    mids = None if exact else mids
    want, want_refs = R.exchange(replicas, refs, block_rows, exact, mids)
    got = run_exchange(device, wire, replicas, refs, block_rows, exact, mids, ranks)
    bad = 0
    for r, (mats, rf) in got.items():
        for k, m in enumerate(mats):
            bad += R.count_differing(m, want[r][k])
            if rf is not None:
                bad += R.count_differing(rf[k], want_refs[r][k])
    return bad, got, (want, want_refs)
