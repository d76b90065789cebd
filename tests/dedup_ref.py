"""The duplicate remover's definition (include/uqhip.h) in plain Python, for the tests: nothing here comes from the
product.  Two independent statements: `rule` is the key / sort / predecessor rule in Python integers, `plain` is what the words mean -- a
dict from compared text to the chosen representative."""
M64 = (1 << 64) - 1
K = 0x9E3779B97F4A7C15
U32 = 0xFFFFFFFF
BEST = 1
FIELDS = ('reads_in', 'bases_in', 'units_in', 'classes', 'dup_units', 'dup_reads', 'dup_bases', 'collisions')
QTAB = bytes(min(max(b - 33, 0), 93) for b in range(256))


def mix(x):
    x &= M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def records(text):
    """The records of a text as lists of their four lines, each without its '\\n'."""
    lines = bytes(text).split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    return [lines[4 * r:4 * r + 4] for r in range((len(lines) - 1) // 4)]


def compared(s, prefix):
    return s if prefix == 0 else s[:prefix]


_DL = {}


def line_hash(c, seed):
    """DL(c) under the seed."""
    got = _DL.get((c, seed))
    if got is not None: return got
    S = mix(seed + K)
    acc = 0
    for k in range((len(c) + 7) // 8):
        w = int.from_bytes(c[8 * k:8 * k + 8], 'little')          # (a short last word is zero-padded by its value)
        acc += mix((w ^ S) + K * (k + 1))
    h = mix((acc & M64) + K * len(c) + 2)
    if len(_DL) < 400000: _DL[(c, seed)] = h
    return h


def unit_hash(texts, seed, hash_bits=64):
    h = line_hash(texts[0], seed) if len(texts) == 1 else mix(line_hash(texts[0], seed) + mix(line_hash(texts[1], seed)))
    return h & ((1 << hash_bits) - 1)


def score(quals):
    return min(sum(sum(u.translate(QTAB)) for u in quals), U32)


def units(text, unit=1, prefix=0, first=0, n=None):
    """[(the compared texts of the unit's records, its quality lines, its sequence lengths)] of the records [first, first + n)."""
    recs = records(text)
    if n is None: n = len(recs) - first
    assert n % unit == 0
    out = []
    for w in range(n // unit):
        mine = recs[first + w * unit:first + (w + 1) * unit]
        out.append((tuple(compared(r[1], prefix) for r in mine), [r[3] for r in mine], [len(r[1]) for r in mine]))
    return out


def key_row(H, sc, w, best):
    return H.to_bytes(8, 'big') + ((U32 - sc).to_bytes(4, 'big') if best else bytes(4)) + w.to_bytes(4, 'big')


def rule(text, unit=1, prefix=0, best=False, seed=0, hash_bits=64, first=0, n=None, index_base=0):
    """The definition as it is written: -> (key rows, verdicts per record, report)."""
    us = units(text, unit, prefix, first, n)
    base = index_base // unit
    rows = [key_row(unit_hash(c, seed, hash_bits), score(q) if best else 0, base + w, best) for w, (c, q, _) in enumerate(us)]
    perm = sorted(range(len(us)), key=lambda w: rows[w])
    rep = dict.fromkeys(FIELDS, 0)
    rep['reads_in'], rep['units_in'] = len(us) * unit, len(us)
    rep['bases_in'] = sum(sum(l) for _, _, l in us)
    v = [0] * (len(us) * unit)
    for j, b in enumerate(perm):
        if j == 0 or rows[perm[j - 1]][:8] != rows[b][:8]:
            rep['classes'] += 1
        elif us[perm[j - 1]][0] == us[b][0]:
            for m in range(unit): v[b * unit + m] = 1
            rep['dup_units'] += 1; rep['dup_reads'] += unit; rep['dup_bases'] += sum(us[b][2])
        else:
            rep['classes'] += 1; rep['collisions'] += 1
    return rows, v, rep


def plain(text, unit=1, prefix=0, best=False, first=0, n=None):
    """What the words mean: of the units with the same compared text one is kept -- the first, or with `best` the one with the highest score,
    ties to the lower index.  -> verdicts per record."""
    us = units(text, unit, prefix, first, n)
    chosen = {}
    for w, (c, q, _) in enumerate(us):
        sc = score(q) if best else 0
        if c not in chosen or sc > chosen[c][0]: chosen[c] = (sc, w)
    keep = {w for _, w in chosen.values()}
    return [0 if w in keep else 1 for w in range(len(us)) for _ in range(unit)]


def kept_text(text, verdicts, unit=1, first=0):
    """The units whose records all have verdict 0, in input order, back to back."""
    recs = records(text)
    out = bytearray()
    for w in range(len(verdicts) // unit):
        if not any(verdicts[w * unit:(w + 1) * unit]):
            for r in recs[first + w * unit:first + (w + 1) * unit]: out += b'\n'.join(r) + b'\n'
    return bytes(out)


def deduped(text, unit=1, prefix=0, best=False):
    """The deduplicated text, by the plain meaning."""
    return kept_text(text, plain(text, unit, prefix, best), unit)
