"""QNAME files for the raw-output tests of uq_qname_tokenise and uq_qname_layout: tests/test_gpu_helpers_exact.py runs them through the
kernels and through the restatements of tests/fake_qname_ops.py, tests/test_qname_device_cpu.py pins on the CPU which of the tokeniser
files are clean and which flag each flagged one raises.  TEST INFRASTRUCTURE ONLY.
A file is (label, prefix_len, suffix_len, separators, names[, expected flag]); every record is name / 'ACGT' / '+' / 'IIII'."""
import numpy as np


TAIL = b'\nACGT\n+\nIIII\n'       # what follows a name: 13 bytes, so only the LAST name of a file can have its 16-byte fetch cross the buffer's end


def byte_tail_lines(names):
    """The names whose staging takes stage_line's byte-by-byte branch (csrc/qname_dev.hip, restated): a line of at most 64 bytes is
    fetched in 16-byte chunks, and a chunk that would read past the end of the buffer is copied byte by byte instead."""
    size, at, out = sum(len(nm) + len(TAIL) for nm in names), 0, []
    for i, nm in enumerate(names):
        if len(nm) <= 64 and any(at + c + 16 > size for c in range(0, len(nm), 16)): out.append(i)
        at += len(nm) + len(TAIL)
    return out


def fastq(names):
    for nm in names:
        assert 10 not in nm
    return np.frombuffer(b''.join(nm + TAIL for nm in names), dtype=np.uint8).copy()


# the fields of the clean files: what int() accepts and what it does not, at the widths where the 8-byte key changes form
FIELDS = [b'', b'0', b'-0', b'+7', b'007', b'-', b'+',
          b'12345678', b'+12345678', b'-12345678', b'123456789', b'+123456789', b'-123456789',                 # 8 and 9 digits
          b'999999999999999999', b'+999999999999999999', b'-999999999999999999', b'100000000000000000',          # 18 digits: +-(10^18 - 1)
          b'abcdefgh', b'abcdefghi', b'ab\x80cd', b'\xff', b'a\x00b', b'\x00', b'12a', b'1-2', b'--1', b'000000000', b'-000000001',
          b'1', b'-5', b'x', b'9' * 17, b'0' * 18]


def _two_columns():
    """'@r' + field + ':' + serial + '/1': every field of FIELDS in column 0, once more in column 1, and a 200-byte name."""
    names = [b'@r' + f + b':' + b'%d' % (1000 + i) + b'/1' for i, f in enumerate(FIELDS)]
    names += [b'@r' + b'%d' % i + b':' + f + b'/1' for i, f in enumerate(FIELDS)]
    names.append(b'@r' + b'y' * 181 + b':' + b'7' * 14 + b'/1')
    assert len(names[-1]) == 200
    names += [b'@r' + b'%d' % (i * i) + b':' + b'%d' % (-i) + b'/1' for i in range(300)]       # more than one workgroup; the last lines are short
    return ('two_columns', 2, 2, b':', names)


def _no_prefix_no_suffix():
    """prefix and suffix of length 0: column 0 starts with the '@' itself; two separators."""
    names = [b'@' + FIELDS[i % len(FIELDS)] + b'_' + FIELDS[(i * 7 + 3) % len(FIELDS)] + b'/' + FIELDS[(i * 5 + 1) % len(FIELDS)]
             for i in range(2 * len(FIELDS))]
    names.append(b'@-1234567_+7/0071')                                                           # 17 bytes, no suffix: its second chunk crosses the buffer's end, and the byte copied alone is the last field's
    assert len(names[-1]) == 17
    return ('no_prefix_no_suffix', 0, 0, b'_/', names)


def _thirty_one_separators():
    """32 columns, names of 100 - 250 bytes (read from HBM, not from the 64-byte LDS row), the longest ones last."""
    seps = bytes(b':/_#|;,='[k % 8] for k in range(31))
    names = []
    for i in range(70):
        fields = [FIELDS[(i + 3 * c) % len(FIELDS)] if (i + c) % 5 == 0 else b'%d' % ((i * 37 + c * 11) % 1000 - 300) for c in range(32)]
        fields[31] += b'z' * (i // 2)
        nm = b'@pre' + b''.join(f + seps[c:c + 1] for c, f in enumerate(fields[:31])) + fields[31] + b'suf'
        assert len(nm) <= 255
        names.append(nm)
    return ('thirty_one_separators', 4, 3, seps, names)


def clean_files():
    return [_two_columns(), _no_prefix_no_suffix(), _thirty_one_separators()]


def flagged_files():
    """Each file is clean but for ONE name (in the middle, and again as the last line) with ONE defect.  The contract sends the caller to
    the host on any flag, so only the flags are compared there."""
    def around(bad):
        good = [b'@r%d:%d.%d/2' % (i, i * 3, 99 - i) for i in range(40)]
        return good[:20] + [bad] + good[20:] + [bad]
    return [('nineteen_digits', 2, 2, b':.', around(b'@r1:1234567890123456789.5/2'), 4),
            ('nineteen_digits_signed', 2, 2, b':.', around(b'@r1:-1000000000000000000.5/2'), 4),
            ('blank_in_field', 2, 2, b':.', around(b'@r1:2 3.5/2'), 2),
            ('tab_in_field', 2, 2, b':.', around(b'@r1:23.\t5/2'), 2),
            ('separator_missing', 2, 2, b':.', around(b'@r1:235/2'), 1),
            ('separator_extra', 2, 2, b':.', around(b'@r1:2.3.5/2'), 1),
            ('separators_out_of_order', 2, 2, b':.', around(b'@r1.2:35/2'), 1),
            ('shorter_than_prefix_and_suffix', 2, 2, b':.', around(b'@r2'), 8)]


# ---- uq_qname_layout: (label, names); line 1 is names[0]
def layout_files():
    rng = np.random.default_rng(5)
    line1 = b'@run7:lane.3:tile_12/x=5 end'
    alpha = np.frombuffer(b'@run7:lane.3tile_12/x=5 endZ09', np.uint8)           # ('Q' is in no line 1: a name that starts with it is no prefix or suffix)

    def noise(n):
        return bytes(rng.choice(alpha, n))
    plain = [line1] + [b'@run7:lane.%d:tile_%d/x=%d end' % (i % 7, i, i % 3) for i in range(400)]
    lengths = [line1] + [b'Q' + noise(L - 1) for L in (1, 2, 15, 16, 17, 63, 64, 65, 66, 127, 200, 254, 255)] + \
              [line1[:10] + noise(L) + line1[-6:] for L in (1, 48, 49, 50, 100, 239)]
    assert max(len(x) for x in lengths) == 255
    prefixes = plain[:30] + [line1[:k] for k in (1, 5, len(line1) - 1)] + plain[30:60]
    suffixes = plain[:30] + [line1[-k:] for k in (1, 4, len(line1) - 1)] + plain[30:60]
    too_long = plain[:50] + [line1[:12] + noise(256 - 12)] + plain[50:90]
    assert len(too_long[50]) == 256
    # a few hundred reads whose LAST lines are the long ones; the very last one is staged and its second 16-byte chunk would cross the
    # end of the buffer (17 bytes + the 13 that follow a name): stage_line copies it byte by byte.  `lengths` ends with a 33-byte one.
    tail = plain[:300] + [line1[:8] + noise(L) for L in (40, 56, 57, 100, 247)] + [b'Q' + noise(L - 1) for L in (64, 50, 33, 16, 3, 17)]
    lengths.append(line1[:12] + noise(21))
    assert len(tail[-1]) == 17 and len(lengths[-1]) == 33
    wide = [bytes(range(48, 48 + 64))] + [bytes(rng.permutation(np.arange(48, 48 + 64)).astype(np.uint8)) for _ in range(20)]   # 64 candidates
    return [('plain', plain), ('lengths', lengths), ('proper_prefixes', prefixes), ('proper_suffixes', suffixes), ('a_name_of_256', too_long),
            ('long_lines_last', tail), ('sixty_four_characters', wide)]
