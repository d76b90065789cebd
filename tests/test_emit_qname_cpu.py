"""The host side of the decoder's QNAME contract, no GPU needed: which integer columns the device may print (stored value + offset inside
[-2**63, 2**64), the offset an int64), that ops._emit_params refuses an offset it cannot hand over, and that the exact host path
(qname.decode_names) such files take equals the oracle at any magnitude."""
import random

import pytest
import torch

import qname_layouts as QL
import uq_oracle as O
from uq_amd import ops, qname, uq


def _config(columns):
    return {'QNAME_columns': columns, 'QNAME_prefix': '@', 'QNAME_suffix': '', 'QNAME_separators': ':' * (len(columns) - 1), 'dna_max': 10}


def _int_col(dtype, mn, mx, offset=True):
    return {'name': 'QNAME_1', 'format': 'integers', 'dtype': dtype, 'min': mn, 'max': mx, 'offset': offset}


@pytest.mark.parametrize('mn', [2 ** 63, 2 ** 64 + 7, -2 ** 63 - 1])
def test_emit_params_refuse_an_offset_beyond_int64(mn):
    cfg = _config([_int_col('uint8', 0, 9, False), _int_col('uint8', mn, mn + 255)])
    with pytest.raises(ValueError, match='QNAME column 2'):
        ops._emit_params(None, cfg, [torch.zeros(4, dtype=torch.uint8)] * 2)


@pytest.mark.parametrize('mn', [-2 ** 63, 2 ** 63 - 1, -25, 0])
def test_emit_params_pass_an_int64_offset_unchanged(mn):
    cfg = _config([_int_col('uint8', mn, mn + 255), _int_col('uint16', mn, mn + 5, False)])
    p = ops._emit_params(None, cfg, [torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int16)])[0]
    assert p.add[0] == mn and p.add[1] == 0                      # no offset: nothing is added, whatever `min` says
    assert (p.ncols, p.itemsize[0], p.itemsize[1]) == (2, 1, 2)


def test_device_text_possible_follows_the_printing_contract():
    ok = uq.Session.device_text_possible
    for mn in (2 ** 63, 2 ** 64 + 7, -2 ** 63 - 1):
        assert not ok(_config([_int_col('uint8', mn, mn + 255)])), mn
    for mn, mx in ((-2 ** 63, -2 ** 63 + 255), (2 ** 63 - 1, 2 ** 63 + 254), (-25, 2 ** 64 - 26), (0, 2 ** 64 - 1)):
        assert ok(_config([_int_col('uint64', mn, mx)])), mn
    assert not ok(_config([_int_col('uint64', 2 ** 63 - 1, 2 ** 64)]))          # the offset fits, the largest sum does not
    assert ok(_config([_int_col('uint64', 0, 2 ** 64 - 1, False)]))
    assert ok(_config([{'name': 'QNAME_1', 'format': 'mapping', 'dtype': 'uint8', 'map': ['a', 'b']}]))
    assert ok(_config([])) and not ok(_config([_int_col('uint8', 0, 9, False)] * 33))
    assert not ok(dict(_config([]), QNAME_prefix='p' * 257))


def _beyond_layouts(n):
    lays = QL.integer_layouts(n, beyond=True)
    r = random.Random(5)
    # offsets no int64 holds: a 20-digit serial number that varies in its last digits, and one past 2**64
    lays['offset=2**63+1'] = QL.layout('@c', '', [QL.int_column('uint8', 2 ** 63 + 1, n, r, True), QL.int_column('uint16', 2 ** 64 + 1, n, r, True),
                                                 QL.int_column('uint64', -2 ** 63 - 1, n, r, True)])
    return lays


def test_host_names_equal_the_oracle_at_any_magnitude():
    """qname.decode_names (Python integers) on the integer layouts of the device tests, with stored values that also print results from
    2**64 on and offsets beyond int64: the path Session.decode takes for files the device declines."""
    cfg0, _, n = QL.tables('T40')
    lays = _beyond_layouts(n)
    seen_beyond = seen_negative = 0
    for name, lay in lays.items():
        cfg, members = QL.craft('T40', lay)
        want = QL.qname_lines(O.decode(cfg, members))
        got = qname.decode_names(cfg, [a for _, a in lay['columns']])
        assert got == want, name
        for c, a in lay['columns']:
            vals = [int(v) + (c['min'] if c['offset'] else 0) for v in a]
            seen_beyond += max(vals) >= 2 ** 64; seen_negative += min(vals) == -2 ** 63
            if name.startswith('offset=2**63') or max(vals) >= 2 ** 64:
                assert not uq.Session.device_text_possible(cfg)
    assert seen_beyond >= 8 and seen_negative >= 4               # the layouts do reach past both ends of the device's range


def test_device_layouts_stay_inside_the_contract():
    """Every integer the device tests print lies in [-2**63, 2**64), every target the issue names is printed by some column, and each
    column stores 0 and the largest value its dtype (or the contract) allows."""
    printed = set()
    for lay in QL.integer_layouts(197).values():
        for c, a in lay['columns']:
            add = c['min'] if c['offset'] else 0
            vals = [int(v) + add for v in a]
            assert -2 ** 63 <= min(vals) and max(vals) < 2 ** 64
            lim = 2 ** (8 * a.dtype.itemsize) - 1
            assert 0 in a.tolist() and int(a.max()) == min(lim, 2 ** 64 - 1 - add)
            printed.update(vals)
        assert uq.Session.device_text_possible({'QNAME_columns': [c for c, _ in lay['columns']], 'QNAME_prefix': '', 'QNAME_suffix': ''})
    assert set(QL.TARGETS) <= printed and -2 ** 63 in printed
