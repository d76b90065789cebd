"""numpy stand-in for dist.HipRows: the row and index operations of one rank on the CPU, following the contracts in
include/uqhip.h.  TEST INFRASTRUCTURE ONLY: tests/test_dist_gloo.py runs the exchange logic of uq_amd.dist on it,
tests/test_gpu_helpers_exact.py holds the routing kernels of csrc/route.hip to it output for output."""
import numpy as np
import torch


class NumpyRows:
    """CPU stand-in for dist.HipRows (stable memcmp row sort, gather, lower bound)."""
    torch = torch
    device = torch.device('cpu')

    def argsort_rows(self, table, rows, cols):
        t = table.numpy().reshape(rows, cols)
        return torch.from_numpy(np.lexsort([t[:, c] for c in range(cols - 1, -1, -1)]).astype(np.int32))

    def argsort_groups(self, table, rows, cols):
        perm = self.argsort_rows(table, rows, cols)
        t = table.numpy().reshape(rows, cols)[perm.numpy().astype(np.int64)]
        head = np.ones(rows, dtype=bool); head[1:] = (t[1:] != t[:-1]).any(axis=1)
        return perm, torch.from_numpy((np.cumsum(head) - 1).astype(np.int32)), int(head.sum())

    def unique_rows_of_groups(self, table, rows, cols, group, nunique, perm=None):
        t = table.numpy().reshape(rows, cols)
        if perm is not None: t = t[perm.numpy().astype(np.int64) & 0xFFFFFFFF]
        g = group.numpy().astype(np.int64)
        first = np.ones(rows, dtype=bool); first[1:] = g[1:] != g[:-1]
        assert int(first.sum()) == nunique
        return torch.from_numpy(np.ascontiguousarray(t[first]).reshape(-1))

    def partition_order(self, dest, n, ndest):
        d = dest.numpy()[:n]
        assert d.max(initial=0) < ndest
        return torch.from_numpy(np.argsort(d, kind='stable').astype(np.int32)), torch.from_numpy(np.bincount(d, minlength=ndest).astype(np.int64))

    def gather_rows(self, table, rows, cols, index):
        t = table.numpy().reshape(rows, cols)
        idx = index.numpy().astype(np.int64) & 0xFFFFFFFF if index.dtype == torch.int32 else index.numpy().astype(np.int64)
        return torch.from_numpy(np.ascontiguousarray(t[idx]).reshape(-1))

    def lower_bound_rows(self, sorted_table, rows, cols, probes, nprobes):
        t = sorted_table.numpy().reshape(rows, cols)
        p = probes.numpy().reshape(nprobes, cols)
        v = lambda a: [bytes(r) for r in a]
        import bisect
        keys = v(t)
        return torch.tensor([bisect.bisect_left(keys, k) for k in v(p)], dtype=torch.int64)

    # the routing arithmetic of csrc/route.hip, restated (include/uqhip.h: uq_partition_rows, uq_owner_of_rows, uq_index_affine,
    # uq_invert_permutation)
    def partition_rows(self, splitters, nsplit, cols, table, rows, index_base, total):
        import bisect
        keys = [bytes(r) for r in splitters.numpy().reshape(nsplit, cols)]
        out = np.zeros(rows, dtype=np.uint8)
        for r, row in enumerate(table.numpy().reshape(rows, cols)):
            lb, ub = bisect.bisect_left(keys, bytes(row)), bisect.bisect_right(keys, bytes(row))
            e = ub - lb
            out[r] = lb + ((index_base + r) * e) // total if e >= 2 else lb
        return torch.from_numpy(out)

    def owner_of_rows(self, gidx, starts):
        s = np.asarray(list(starts), dtype=np.int64)
        return torch.from_numpy((np.searchsorted(s[1:-1], gidx.numpy(), side='right')).astype(np.uint8))

    def index_affine(self, index, add, out_itemsize):
        a = index.numpy().astype(np.int64)
        if index.dtype == torch.int32: a &= 0xFFFFFFFF
        return torch.from_numpy((a + add).astype(np.int32 if out_itemsize == 4 else np.int64))

    def scatter_rows(self, values, n, cols, index, base, out_rows):
        a = index.numpy().astype(np.int64)
        if index.dtype == torch.int32: a &= 0xFFFFFFFF
        a = a - base
        assert sorted(a.tolist()) == list(range(out_rows))
        out = np.empty((out_rows, cols), dtype=np.uint8)
        out[a] = values.numpy().reshape(n, cols)
        return torch.from_numpy(out.reshape(-1))

    def invert_permutation(self, perm, base=0):
        a = perm.numpy().astype(np.int64)
        if perm.dtype == torch.int32: a &= 0xFFFFFFFF
        a = a - base
        assert sorted(a.tolist()) == list(range(len(a)))
        inv = np.empty(len(a), dtype=np.int32)
        inv[a] = np.arange(len(a), dtype=np.int32)
        return torch.from_numpy(inv)
