#!/usr/bin/env python3
"""The text fixtures of the larger cases are committed gzip-compressed (<name>.fastq.gz, <name>.refdecode.fastq.gz): a binary
file of a third of the size instead of a few hundred thousand lines of FASTQ in a diff.  inflate() writes the plain files the
tests read next to them (git ignores those); __graft_entry__.build() calls it.  `--pack <name> ...` makes the committed form
from the plain files tests/golden/make_golden.py wrote (gzip level 9, no name, no time: the same bytes every time)."""
import glob
import gzip
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def inflate(directory=HERE):
    """<x>.fastq.gz -> <x>.fastq wherever the plain file is missing or holds other bytes; returns the plain paths."""
    out = []
    for gz in sorted(glob.glob(os.path.join(directory, '*.fastq.gz'))):
        plain = gz[:-3]
        data = gzip.decompress(open(gz, 'rb').read())
        if not os.path.exists(plain) or open(plain, 'rb').read() != data:
            tmp = '%s.tmp.%d' % (plain, os.getpid())
            with open(tmp, 'wb') as f: f.write(data)
            os.replace(tmp, plain)
        out.append(plain)
    return out


def pack(names, directory=HERE):
    for name in names:
        for ext in ('.fastq', '.refdecode.fastq'):
            plain = os.path.join(directory, name + ext)
            if os.path.exists(plain):
                with open(plain + '.gz', 'wb') as f: f.write(gzip.compress(open(plain, 'rb').read(), 9, mtime=0))


if __name__ == '__main__':
    if sys.argv[1:2] == ['--pack']: pack(sys.argv[2:])
    else: print('\n'.join(inflate()))
