"""The reference of quality binning (`--bin-qual`), in numpy: a 256-entry table applied to line 4 of every record of a FASTQ text.
TEST INFRASTRUCTURE ONLY: uq_requantise_qualities (device) and uq_requantise_qualities_host are held to this."""
import numpy as np

from uq_amd import ops


def apply(data, lut, first_read=0, nreads=None):
    """(the text with lut applied to the quality lines of records [first_read, first_read + nreads), as bytes; bytes changed)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    ls = ops.host_line_starts(a).astype(np.int64)
    if nreads is None: nreads = (len(ls) - 1) // 4 - first_read
    table = np.frombuffer(bytes(lut), dtype=np.uint8)
    mask = np.zeros(len(a) + 1, dtype=np.int32)
    r = np.arange(first_read, first_read + nreads)
    np.add.at(mask, ls[4 * r + 3], 1)                   # +1 at the first quality byte, -1 at the line's newline: a running sum marks the lines
    np.add.at(mask, ls[4 * r + 4] - 1, -1)
    own = np.cumsum(mask[:-1]) > 0
    new = np.where(own, table[a], a)
    return new.tobytes(), int(np.count_nonzero(new != a))


IDENTITY = bytes(range(256))
ALL_I = b'I' * 256                                      # hostile: every byte, newlines included, would become 'I' wherever the table is applied
