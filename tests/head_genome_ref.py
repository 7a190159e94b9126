"""`head-genome` restated in plain Python (PARITY.md HEADG; the loop is bigseqkit-lib/head_genome.go:53-108).

    words(Desc)  the maximal runs of bytes other than ' ' and '\\t' (stringutil.Split(Desc, "\\t "): no empty words)
    prefix       words(Desc of record 0)
    n_i          the number of leading words of record i equal to the prefix's, up to the shorter list
    cut c        the lowest i >= 1 with n_i < m or n_i != n_1; none: the record count.  Records 0 .. c-1 are kept
    a kept record with len(Desc) == 0 (the lowest one) fails the call: "no description: <ID>"

What a record IS comes from the oracle (record_spans), ID / Desc from the oracle's parseHeadIDAndDesc (parse_head), and the
kept text is the oracle's `seq` without options on the bytes in front of the cut."""
import json
import re

import oracle

NCBI = r"\|([^\|]+)\| "


class HeadGenomeError(Exception):
    pass


def words(desc):
    return [w for w in re.split(rb"[\t ]+", bytes(desc)) if w]


def shared(ws, prefix):
    n = 0
    for a, b in zip(ws, prefix):
        if a != b:
            break
        n += 1
    return n


def verdicts(descs, m=1):
    """descs: Desc of every record, in order -> (cut index, error or None).  The loop as written for m >= 1."""
    if m < 1:
        raise HeadGenomeError("value of flag --mini-common-words should be greater than 0")
    prefix, n1 = None, None
    for i, d in enumerate(descs):
        if len(d) == 0:
            return i, i  # (head_genome.go:68-70 runs before everything else)
        if prefix is None:
            prefix = words(d)
            continue
        n = shared(words(d), prefix)
        if n < m:
            return i, None
        if n1 is None:
            n1 = n
        elif n != n1:
            return i, None
    return len(descs), None


def heads(data, fastq, regexp=""):
    """[(start, ID, Desc)] of the records of `data`"""
    data = bytes(data)
    out = []
    for s, ln in oracle.record_spans(data, fastq):
        head = data[s + 1:s + ln].split(b"\n", 1)[0]
        i, d = oracle.parse_head(head.decode("latin-1"), regexp)
        out.append((s, i.encode("latin-1"), d.encode("latin-1")))
    return out


def cut_byte(data, fastq, m=1, regexp=""):
    """the byte where the first record that is NOT kept begins (len(data): every record is kept)"""
    hs = heads(data, fastq, regexp)
    c, bad = verdicts([d for _, _, d in hs], m)
    if bad is not None:
        raise HeadGenomeError("no description: " + hs[bad][1].decode("latin-1"))
    return (hs[c][0] if c < len(hs) else len(data)), c


def head_genome(data, fastq, m=1, line_width=60, regexp=""):
    data = bytes(data)
    if m < 1:
        raise HeadGenomeError("value of flag --mini-common-words should be greater than 0")
    if not oracle.record_spans(data, fastq):
        return b""
    cb, _ = cut_byte(data, fastq, m, regexp)
    cfg = {"LineWidth": line_width}
    if regexp:
        cfg["IDRegexp"] = regexp
    return oracle.seq(data[:cb], fastq, json.dumps({"Config": cfg}))
