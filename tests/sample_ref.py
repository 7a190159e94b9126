"""`sample` and `shuffle` restated in plain Python (PARITY.md SAMPLE, SHUF; driver arithmetic bigseqkit/sample.go:55-73).

    draw(seed, g) = splitmix64(splitmix64((uint64)(int64)seed) ^ g)        g = 0-based index of the record in the whole input
    sample:  record g is kept iff (draw(seed, g) >> 11) < T,  T = ceil(fraction * 2^53)
    shuffle: the records in ascending order of draw(seed, g)

The draw is defined on Python integers (no numpy).  What a record IS comes from the oracle (RECTEXT: the element
PlainFile + ReadFixer hand over, as `range` / `duplicate` print it), not from here."""
import math
import struct

import oracle

M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, g):
    return splitmix64(splitmix64(seed & M64) ^ g)


def f32(p):
    """float64(float32(p)): Proportion is a float32 in the reference's options"""
    return struct.unpack("<f", struct.pack("<f", p))[0]


class SampleError(Exception):
    pass


def fraction(number=0, proportion=0.0, count=None):
    """bigseqkit/sample.go:55-73 as written; `count` = input.Count(), looked at only when number > 0"""
    p = f32(proportion)
    if number == 0 and p == 0:
        raise SampleError("one of flags -n (--number) and -p (--proportion) needed")
    if number < 0:
        raise SampleError("value of -n (--number) and should be greater than 0")
    if p < 0 or p > 1:
        raise SampleError("value of -p (--proportion) (%f) should be in range of (0, 1]" % p)
    if number > 0:
        return float(number) / float(count) if count else math.inf  # (Go: a float division by zero is +Inf, no error)
    return p


def threshold(frac):
    if not frac < 1.0:
        return 1 << 53
    if frac <= 0.0:
        return 0
    return math.ceil(frac * 9007199254740992.0)  # exact: a scaling by 2^53


def keeps(seed, g, T):
    return (draw(seed, g) >> 11) < T


def kept_indices(seed, n, T, first=0):
    return [i for i in range(n) if keeps(seed, first + i, T)]


def shuffle_order(seed, n):
    return sorted(range(n), key=lambda g: draw(seed, g))


def records(data, fastq):
    """the record texts (no final newline) of `data`, by the oracle's ReadFixer"""
    data = bytes(data)
    return [data[s:s + ln] for s, ln in oracle.record_spans(data, fastq)]


def sample(data, fastq, seed=11, number=0, proportion=0.0, first=0, count=None):
    recs = records(data, fastq)
    T = threshold(fraction(number, proportion, len(recs) if count is None else count))
    return b"".join(recs[i] + b"\n" for i in kept_indices(seed, len(recs), T, first))


def shuffle(data, fastq, seed=23):
    recs = records(data, fastq)
    return b"".join(recs[i] + b"\n" for i in shuffle_order(seed, len(recs)))
