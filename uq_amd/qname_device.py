"""QNAME passes with the per-read work on the device (device form).

The reference's loop over QNAME lines (uq.py:394-444, 555-678, 717-736) keeps order-dependent state,
but every decision it takes is a function of a few reductions over the reads (see csrc/qname_dev.hip).
This module runs those reductions / the tokeniser through the C ABI and finishes the decisions on the
host, on a handful of numbers per column.  It reproduces the reference only for inputs inside an
exactly-characterised subset (ASCII fields, plain decimal integers, separators that are not regex
metacharacters, ...); outside it `analyse_device` returns None and the caller uses the sequential
host implementation (`qname.analyse_native` / `qname.analyse`).  The column arrays stay in HBM.

Sharded input (one rank per GPU, `shard` = uq_amd.dist.Shard): every reduction is combined over the
ranks with MIN / MAX / SUM of a few integers, the distinct counts come from a distributed sort of the
8-byte field keys, and all ranks reach the same decisions (or the same refusal) from the same numbers.
"""
import numpy as np

from . import ops
from ._lib import UQ_NONE, UqHipError
from .qname import QnameError, _LADDER

# '[' + seps + ']+' and '(.*)'.join(seps) are regexes in the reference: leave their metacharacters to `re`
REGEX_SPECIAL = frozenset('.^$*+?{}[]\\|()-')
_STRINGS = 'Encoding QNAMEs as strings has not been implimented yet.'
_I64_MAX = (1 << 63) - 1
INT_RANGE_SMALL = 4096          # value ranges counted over the whole column (private LDS tables)
INT_RANGE_MAX = 1 << 24         # widest range the sort-free count is tried on
INT_PREFIX = 1 << 21            # reads a wide-range column is judged on before the sort is paid for


def _ladder(x):
    for lim, dt in _LADDER:
        if x <= lim:
            return lim, dt
    return None, None


def _thresholds(n):
    """The reads after which the reference re-examines its column formats (uq.py:586-602: 10 000, 20 000, 40 000, ...) and the last one
    (uq.py:634-638), as 0-based read numbers."""
    thresholds = []
    t = 10000
    while t <= n - 1:
        thresholds.append(t); t *= 2
    if not thresholds or thresholds[-1] != n - 1:
        thresholds.append(n - 1)
    return thresholds


def _fetch_bytes(ctx, d_buf, lo, hi):
    return ctx.to_numpy(d_buf[lo:hi]).tobytes()


def _min_u64(shard, values):
    """MIN over ranks of unsigned values where UQ_NONE means 'none' (read numbers stay below 2^63)."""
    if shard is None or shard.world == 1:
        return list(values)
    red = shard.reduce([_I64_MAX if v == UQ_NONE else v for v in values], 'min')
    return [UQ_NONE if v == _I64_MAX else v for v in red]


def infer_layout_device(ctx, d_buf, d_ls, nreads, shard=None):
    """uq.py:348-352, 394-413, 428-444 -> (prefix, suffix, separators) as latin-1 strings, or None."""
    base = shard.read_offset if shard else 0
    head = _fetch_bytes(ctx, d_buf, 0, min(257, d_buf.numel())) if nreads else b''
    if shard is not None:
        head = shard.gather_bytes(head if shard.rank == 0 else b'')[0]        # line 1 of the whole file
    nl = head.find(b'\n')
    if nl < 0:
        return None
    line1 = head[:nl]
    if not line1.startswith(b'@'):
        raise QnameError('ERROR: This does not look like a FASTA/FASTQ file! (first line does not start with @)')
    if len(line1) > 255:
        return None
    try:
        res = ops.qname_layout(ctx, d_buf, d_ls, nreads, line1, base)
    except UqHipError:
        return None                      # more than 64 distinct characters in line 1
    nch = res.nch
    flags, plen, slen = res.flags, res.min_lcp, res.min_lcs
    entry, lastviol = list(res.entry[:nch]), list(res.lastviol[:nch])
    if shard is not None and shard.world > 1:
        plen, slen = shard.reduce([plen, slen], 'min')
        red = shard.reduce([flags] + lastviol, 'max')
        flags, lastviol = red[0], red[1:]
        entry = _min_u64(shard, entry)
    if flags:
        return None
    l1 = line1.decode('latin-1')
    prefix = l1[:plen]
    suffix = l1[len(l1) - slen:] if slen else ''
    seps = set()
    for k in range(nch):
        if entry[k] != UQ_NONE and lastviol[k] < entry[k]:
            c = chr(res.ch[k])
            if l1[plen:].count(c) - suffix.count(c) != 0:
                seps.add(c)
    if not seps:
        raise QnameError('ERROR: the QNAMEs share no constant-count separator; the reference cannot encode such '
                         'files either (SURVEY.md Q13)')
    if seps & REGEX_SPECIAL or plen + slen > len(l1):
        return None
    last = b''
    if nreads:
        o = ctx.to_numpy(d_ls[4 * (nreads - 1):4 * (nreads - 1) + 2], np.uint64)
        last = _fetch_bytes(ctx, d_buf, int(o[0]), int(o[1]) - 1)
    if shard is not None:
        last = [b for b in shard.gather_bytes(last + b'\n' if nreads else b'') if b][-1][:-1]   # the last QNAME of the whole file
    last = last.decode('latin-1')

    def order_seps(q):
        return ''.join(ch for ch in q[plen:-1 - slen] if ch in seps)

    if order_seps(last) != order_seps(l1):
        raise QnameError("ERROR: Sorry, the separators used in this file's QNAME/headers are so unusual/improbable "
                         "that the reference gives up; so does this implementation")
    separators = order_seps(last)
    if not 1 <= len(separators) <= 31:
        return None
    return prefix, suffix, separators


def _distinct_counts(ctx, keys, n, thresholds, shard):
    """-> (distinct-count among reads [0, T] for each T, number of distinct keys, key codes tensor or None,
    sorted unique rows tensor [nu * 8]).  Codes (rank of each read's key) are only produced on one GPU;
    sharded callers look them up in the gathered unique table."""
    if shard is None or shard.world == 1:
        perm, key, skey, uniq, nu = ops.unique_rows(ctx, keys, n, 8)
        return ops.prefix_distinct(ctx, perm, skey, n, thresholds), nu, key, uniq
    from .dist import global_sort_rows
    gs = global_sort_rows(shard.be, keys.view(ctx.torch.uint8), n, 8, shard.read_offset, shard.group, total_rows=shard.total, want='unique')
    m = gs['rows']
    counts, nu, uniq, edge, first0 = [0] * len(thresholds), 0, ctx.empty(0), b'', 0
    if m:
        skey, nu = gs['group'], gs['ngroups']                # the shard came out of the sort in order, with its groups
        uniq = gs['unique']
        counts = ops.prefix_distinct(ctx, gs['gidx'], skey, m, thresholds)           # gidx = file-wide read numbers, ascending inside a group
        edge = bytes(ctx.to_numpy(gs['edge']).tobytes())
        first0 = int(ctx.to_numpy(gs['gidx'][:1], np.int64)[0])          # the shard's first row is the first of its group in file order (stable sort)
    # Equal keys share a rank -- except a value heavier than a rank's share, which global_sort_rows deals over several ranks by file
    # position.  Such a group is counted by every rank that holds a piece of it; its true first occurrence sits on the EARLIEST of them.
    # So a rank whose first key equals the last key in front of it (first + last row of every rank, as dist_encode._unique does) drops
    # that row from its unique slice and takes the group off nu and off every checkpoint at or after its own first occurrence of it.
    edges = shard.gather_bytes(edge)
    last, cont = None, 0
    for r in range(shard.world):
        if r == shard.rank: cont = 1 if (edges[r] and last is not None and edges[r][:8] == last) else 0
        if edges[r]: last = edges[r][8:]
    if cont:
        uniq, nu = uniq[8:], nu - 1
        counts = [c - (1 if first0 <= T else 0) for c, T in zip(counts, thresholds)]
    red = shard.reduce(list(counts) + [nu], 'sum')
    return red[:-1], red[-1], None, shard.gather_rows(uniq)


def type_and_encode_device(ctx, d_buf, d_ls, nreads, prefix, suffix, separators, shard=None):
    """uq.py:555-678 + 717-736 -> (columns, device column tensors) or None."""
    n_local = nreads
    n = shard.total if shard else nreads                     # reads in the whole file
    base = shard.read_offset if shard else 0
    vals, strs, res = ops.qname_tokenise(ctx, d_buf, d_ls, n_local, len(prefix), len(suffix), separators.encode('latin-1'))
    ncols = len(separators) + 1
    flags = res.flags
    first_nonint = [UQ_NONE if res.first_nonint[c] == UQ_NONE else res.first_nonint[c] + base for c in range(ncols)]
    vmins, vmaxs = list(res.vmin[:ncols]), list(res.vmax[:ncols])
    long_bad = [res.any_long[c] & 1 for c in range(ncols)]
    long_int = [(res.any_long[c] >> 1) & 1 for c in range(ncols)]
    if shard is not None and shard.world > 1:
        red = shard.reduce([flags] + vmaxs + long_bad + long_int, 'max')
        flags, vmaxs, long_bad, long_int = red[0], red[1:1 + ncols], red[1 + ncols:1 + 2 * ncols], red[1 + 2 * ncols:]
        vmins = shard.reduce(vmins, 'min')
        first_nonint = _min_u64(shard, first_nonint)
    if flags:
        return None
    thresholds = _thresholds(n)
    columns, arrays = [], []
    for c in range(ncols):
        if long_bad[c]:
            return None
        col = {'name': 'QNAME_%d' % (c + 1), 'format': 'mapping'}
        all_int = first_nonint[c] == UQ_NONE
        vmin, vmax = vmins[c], vmaxs[c]
        counts = None
        key = uniq = None
        # An all-integer column whose fields are the canonical decimals of their values has as many distinct strings as
        # distinct VALUES: first occurrences per value (atomic minima over [vmin, vmax]) give every checkpoint's count
        # without the sort (uq_int_prefix_distinct).  Small ranges are settled for the whole column; wide ones (flow-cell
        # coordinates) from a prefix of the reads, where the `len(map) > entries_read / 10` rule fires at once or never.
        value_range = vmax - vmin + 1 if all_int else 0
        if (shard is None or shard.world == 1) and all_int and not (res.any_long[c] & 4) and 1 <= value_range <= INT_RANGE_MAX:
            if value_range <= INT_RANGE_SMALL:
                counts = ops.int_prefix_distinct(ctx, vals[c], n_local, vmin, value_range, thresholds)
                nu = counts[-1]
            else:
                head = [T for T in thresholds if T < INT_PREFIX]
                if head:
                    hc = ops.int_prefix_distinct(ctx, vals[c], min(n_local, head[-1] + 1), vmin, value_range, head)
                    if any(cnt > T // 10 for T, cnt in zip(head, hc)): counts, nu = hc, None      # demoted inside the prefix: nu is not needed
                    elif len(head) == len(thresholds): counts, nu = hc, hc[-1]                    # the prefix was the whole column
        if counts is None:
            counts, nu, key, uniq = _distinct_counts(ctx, strs[c], n_local, thresholds, shard)
        for T, cnt in zip(thresholds, counts):
            if cnt > T // 10:                               # check_format(): mapping -> integers
                if not all_int:
                    raise QnameError(_STRINGS)
                col['format'] = 'integers'
                break
        if col['format'] == 'mapping' and uniq is None and not (all_int and vmax - vmin <= _ladder(nu)[0]):
            counts, nu, key, uniq = _distinct_counts(ctx, strs[c], n_local, thresholds, shard)     # it stays a mapping: the sorted map is needed
        if col['format'] == 'mapping':
            lim, dt = _ladder(nu)
            col['dtype'] = dt
            if all_int and vmax - vmin <= lim:
                col['format'] = 'integers'; col['max'] = vmax; col['min'] = vmin
                col['offset'] = bool(vmin < 0 or vmax > lim)
            else:
                if long_int[c]:
                    return None                             # sorted map of strings longer than the 8-byte key
                rows = ctx.to_numpy(uniq).reshape(nu, 8)
                col['map'] = [s.decode('latin-1') for s in np.ascontiguousarray(rows).view('S8').ravel().tolist()]
        else:
            col['min'] = vmin; col['max'] = vmax
            lim, dt = _ladder(vmax - vmin)
            col['dtype'] = dt
            col['offset'] = bool(vmin < 0 or vmax > lim)
        isz = np.dtype(col['dtype']).itemsize
        if col['format'] == 'mapping':
            if key is None:                                 # sharded: rank of each key in the gathered sorted map
                key = ops.lower_bound_rows(ctx, uniq, nu, 8, strs[c], n_local).to(ctx.torch.int32)
            arrays.append(ops.narrow(ctx, key, isz))
        else:
            arrays.append(ops.encode_int(ctx, vals[c], col['min'] if col['offset'] else 0, isz))
        columns.append(col)
        vals[c] = strs[c] = None                            # release this column's staging as we go
    return columns, arrays


DECLINE, NEEDS_SORT = 'decline', 'needs sort'
_DT_OF_ITEMSIZE = {1: 'uint8', 2: 'uint16', 4: 'uint32', 8: 'uint64'}


def fused_columns_py(r, n, sorted_counts=None):
    """The column typing of uq.py:586-678 from a fetched uq_qname_fused `r` for n reads: the list of column descriptions, DECLINE (the
    fused pass cannot vouch for the file: no guess, a flag, another read count or other checkpoints, a column that stays a mapping of
    strings) or NEEDS_SORT (a column's distinct counts have to come from a sort of its values: sorted_counts(c) -> (counts at every
    checkpoint, distinct values), when given, supplies them).  The Python twin of uq_qname_fused_columns (csrc/decide.hip), which
    analyse_fused runs; the tests compare the two."""
    if not r.ok or r.flags or n == 0 or int(r.nreads) != n:
        return DECLINE
    thresholds = _thresholds(n)
    if list(r.thresholds[:r.nth]) != thresholds:
        return DECLINE
    columns = []
    for c in range(r.nsep + 1):
        vmin, vmax = int(r.vmin[c]), int(r.vmax[c])
        col = {'name': 'QNAME_%d' % (c + 1), 'format': 'mapping'}
        # every field is the canonical decimal of its value (the kernel verified it): distinct strings = distinct values, counted per
        # checkpoint from first occurrences -- over the whole column for small ranges, else over the checkpoints below INT_PREFIX,
        # where the `len(map) > entries_read / 10` rule fires at once or the values are sorted (type_and_encode_device's rule)
        counts = None
        if not r.undetermined[c] and vmax - vmin + 1 <= INT_RANGE_SMALL:
            ths, counts = thresholds, r.counts[c][:len(thresholds)]
            nu = counts[-1]
        elif not r.undetermined[c]:
            ths = [T for T in thresholds if T < INT_PREFIX]
            counts = r.counts[c][:len(ths)]
            if any(cnt > T // 10 for T, cnt in zip(ths, counts)): nu = None
            elif len(ths) == len(thresholds): nu = counts[-1]
            else: counts = None
        if counts is None:                                  # a stable sort of the 4-byte values (any order will do for counting)
            if sorted_counts is None:
                return NEEDS_SORT
            ths = thresholds
            counts, nu = sorted_counts(c)
        for T, cnt in zip(ths, counts):
            if cnt > T // 10:                               # check_format(): mapping -> integers
                col['format'] = 'integers'
                break
        if col['format'] == 'mapping':
            lim, dt = _ladder(nu)
            col['dtype'] = dt
            if vmax - vmin > lim:
                return DECLINE                              # stays a mapping: the sorted map of its strings comes from the exact path
            col['format'] = 'integers'; col['max'] = vmax; col['min'] = vmin
            col['offset'] = bool(vmax > lim)
        else:
            col['min'] = vmin; col['max'] = vmax
            lim, dt = _ladder(vmax - vmin)
            col['dtype'] = dt
            col['offset'] = bool(vmax > lim)
        columns.append(col)
    return columns


def fused_columns(r, n):
    """uq_qname_fused_columns: the same answer as fused_columns_py(r, n) from the library."""
    import ctypes as C
    from ._lib import QnameColumns, call
    out = QnameColumns()
    call('uq_qname_fused_columns', C.byref(r), int(n), C.byref(out))
    if out.status:
        return DECLINE if out.status == 1 else NEEDS_SORT
    columns = []
    for c in range(out.ncols):
        dt = _DT_OF_ITEMSIZE[out.itemsize[c]]
        if out.from_mapping[c]:
            columns.append({'name': 'QNAME_%d' % (c + 1), 'format': 'integers', 'dtype': dt, 'max': out.vmax[c], 'min': out.vmin[c], 'offset': bool(out.offset[c])})
        else:
            columns.append({'name': 'QNAME_%d' % (c + 1), 'format': 'integers', 'min': out.vmin[c], 'max': out.vmax[c], 'dtype': dt, 'offset': bool(out.offset[c])})
    return columns


def analyse_fused(ctx, fq, nreads):
    """The QNAME analysis from what the pack kernel's QNAME phase left behind (ops.FusedQname after pack_stats(fq=...) and
    qname_fused_finish): (prefix, suffix, separators, columns, device column tensors), or None when the fused pass cannot vouch for
    it -- the guess declined, a read did not conform (any flag), a column needs the sorted map -- and the caller runs analyse_device.
    One host wait (the fetch); the columns are typed in the library (uq_qname_fused_columns) and their encoders queued behind it.  A
    column whose distinct counts need a sort of its values goes through the Python rules, with the sort."""
    r = ops.qname_fused_fetch(ctx, fq)
    n = int(nreads)
    columns = fused_columns(r, n)
    if columns == NEEDS_SORT:
        def sorted_counts(c):
            perm, _, skey, _, nu = ops.unique_rows(ctx, fq.column(c, n).view(ctx.torch.uint8), n, 4, want_key=False, want_unique=False)
            return ops.prefix_distinct(ctx, perm, skey, n, _thresholds(n)), nu
        columns = fused_columns_py(r, n, sorted_counts)
    if columns == DECLINE:
        return None
    l1 = bytes(r.line1[:r.l1len]).decode('latin-1')
    prefix = l1[:r.plen]
    suffix = l1[r.l1len - r.slen:] if r.slen else ''
    separators = bytes(r.seps[:r.nsep]).decode('latin-1')
    arrays = ops.encode_u32_columns(ctx, fq, n, [c['min'] if c['offset'] else 0 for c in columns], [np.dtype(c['dtype']).itemsize for c in columns])
    return prefix, suffix, separators, columns, arrays


def broadcast_guess(ctx, fq, shard):
    """The fused pass over shards, step 1: rank 0's layout guess (ops.qname_guess[_async] has been queued on rank 0) becomes every rank's --
    the structure's bytes travel in ONE broadcast, queued on the stream like any kernel (nccl); the pack kernels behind it verify the
    layout on every read of every shard."""
    if shard is None or shard.world == 1:
        return
    dist = shard.dist
    if dist.get_backend(shard.group) == 'gloo' and fq.q.is_cuda:
        host = fq.q.cpu(); dist.broadcast(host, src=0, group=shard.group); fq.q.copy_(host)      # rehearsal with ranks sharing a card
    else:
        dist.broadcast(fq.q, src=0, group=shard.group)


def analyse_fused_sharded(ctx, fq, nreads, shard, usable=True):
    """analyse_fused for one rank of a sharded file (`nreads` = this rank's reads, shard = uq_amd.dist.Shard): the layout was rank 0's guess
    (broadcast_guess), every rank's pack kernel verified it on its own reads and ran its local qname_fused_finish.  Combined here:
      * ok / flags / read counts / vmin / vmax of all ranks, and rank 0's early-checkpoint counts of the wide-range columns (reads
        [0, 40 000] are rank 0's), in ONE all-gather of a few integers per rank;
      * the small-range columns' first-occurrence tables (file-wide read numbers) in ONE all-reduce (MIN): the distinct counts at every
        checkpoint of the FILE follow (uq.py:586-602, 634-638).
    Every rank takes the same decisions from the same numbers, and every rank MUST call this (it is collective): a rank whose own pass is
    not usable -- no speculative pack, a declined guess, tables beyond their capacity -- passes usable=False and says so in the all-gather.
    None: some rank raised a flag, a column stays undecided (it would need
    the distributed sort of its values) or a mapping of strings -- the caller runs analyse_device(shard=...), the exact sharded kernels."""
    if shard is None or shard.world == 1:
        return analyse_fused(ctx, fq, nreads) if (usable and fq is not None) else None
    t = ctx.torch
    n = int(nreads)
    MAXC = 8
    if usable and fq is not None:
        r = ops.qname_fused_fetch(ctx, fq)
        mine = [int(bool(r.ok)), int(r.flags != 0 or int(r.nreads) != n), n, int(r.nsep)]
        mine += [int(r.vmin[c]) for c in range(MAXC)] + [int(r.vmax[c]) for c in range(MAXC)] + [int(r.undetermined[c]) for c in range(MAXC)]
        mine += [int(r.counts[c][k]) for c in range(MAXC) for k in range(3)]
    else:
        mine = [0, 1, n, 0] + [0] * (3 * MAXC + 3 * MAXC)
    flat = [0] * (len(mine) * shard.world)
    flat[shard.rank * len(mine):(shard.rank + 1) * len(mine)] = mine
    allv = shard.reduce(flat, 'sum')
    allv = [allv[q * len(mine):(q + 1) * len(mine)] for q in range(shard.world)]
    have = [v for v in allv if v[2] > 0]                                   # ranks with reads
    if not allv[0][0] or allv[0][2] == 0 or any(v[1] for v in have) or sum(v[2] for v in allv) != shard.total:
        return None
    ncols = allv[0][3] + 1
    N = shard.total
    thresholds = _thresholds(N)
    gvmin = [min(v[4 + c] for v in have) for c in range(ncols)]
    gvmax = [max(v[12 + c] for v in have) for c in range(ncols)]
    n0 = allv[0][2]
    small = [c for c in range(ncols) if gvmax[c] - gvmin[c] + 1 <= INT_RANGE_SMALL]
    counts_small = {}
    if small:
        ranges = [gvmax[c] - gvmin[c] + 1 if c in small else 0 for c in range(ncols)]
        first = ops.qname_fused_first_seen(ctx, fq, n, shard.read_offset, gvmin, ranges)
        if shard.dist.get_backend(shard.group) == 'gloo' and first.is_cuda:
            host = first.cpu(); shard.dist.all_reduce(host, op=shard.dist.ReduceOp.MIN, group=shard.group)
        else:
            shard.dist.all_reduce(first, op=shard.dist.ReduceOp.MIN, group=shard.group); host = first.cpu()
        tab = host.numpy().reshape(MAXC, 4096)
        for c in small:
            row = tab[c][:ranges[c]]
            counts_small[c] = [int((row <= T).sum()) for T in thresholds]
    head = [T for T in thresholds if T < INT_PREFIX][:3]                   # the checkpoints the wide-range kernel looks at (qf_wide_part)
    columns = []
    for c in range(ncols):
        vmin, vmax = gvmin[c], gvmax[c]
        col = {'name': 'QNAME_%d' % (c + 1), 'format': 'mapping'}
        if c in counts_small:
            ths, counts = thresholds, counts_small[c]
            nu = counts[-1]
        else:
            # rank 0 judged the column on reads [0, T], T = 10 000, 20 000, 40 000: the file's own first checkpoints when rank 0 holds them
            # all and ran its wide-range kernel on this column; it fires there (flow-cell coordinates do) or the column stays undecided
            r0 = allv[0]
            if not head or n0 <= head[-1] or r0[12 + c] - r0[4 + c] + 1 <= INT_RANGE_SMALL or _thresholds(n0)[:len(head)] != head:
                return None
            ths, counts = head, [r0[28 + 3 * c + k] for k in range(len(head))]
            fired = [k for k, (T, cnt) in enumerate(zip(ths, counts)) if cnt > T // 10]
            if not fired:
                return None
            ths, counts, nu = ths[:fired[0] + 1], counts[:fired[0] + 1], None
        for T, cnt in zip(ths, counts):
            if cnt > T // 10:
                col['format'] = 'integers'
                break
        if col['format'] == 'mapping':
            lim, dt = _ladder(nu)
            col['dtype'] = dt
            if vmax - vmin > lim:
                return None                                 # stays a mapping of strings: the exact path's sorted map
            col['format'] = 'integers'; col['max'] = vmax; col['min'] = vmin
            col['offset'] = bool(vmax > lim)
        else:
            col['min'] = vmin; col['max'] = vmax
            lim, dt = _ladder(vmax - vmin)
            col['dtype'] = dt
            col['offset'] = bool(vmax > lim)
        columns.append(col)
    l1 = bytes(r.line1[:r.l1len]).decode('latin-1')
    prefix = l1[:r.plen]
    suffix = l1[r.l1len - r.slen:] if r.slen else ''
    separators = bytes(r.seps[:r.nsep]).decode('latin-1')
    arrays = ops.encode_u32_columns(ctx, fq, n, [c['min'] if c['offset'] else 0 for c in columns], [np.dtype(c['dtype']).itemsize for c in columns]) if n else \
        [ctx.torch.empty(0, dtype=getattr(t, {1: 'uint8', 2: 'int16', 4: 'int32', 8: 'int64'}[np.dtype(c['dtype']).itemsize]), device=ctx.device) for c in columns]
    return prefix, suffix, separators, columns, arrays


def analyse_device(ctx, d_buf, d_ls, nreads, shard=None):
    """(prefix, suffix, separators, columns, device column tensors), or None -> use the host path."""
    lay = infer_layout_device(ctx, d_buf, d_ls, nreads, shard)
    if lay is None:
        return None
    prefix, suffix, separators = lay
    out = type_and_encode_device(ctx, d_buf, d_ls, nreads, prefix, suffix, separators, shard)
    if out is None:
        return None
    return prefix, suffix, separators, out[0], out[1]
