"""`fa2fq` in plain Python, as PARITY.md FA2FQ fixes it: what bigseqkit-lib/fa2fq.go:59-120 documents (the reference's
loop drops its plus-strand hits and appends an empty string for every miss; that is not reproduced).  The FASTA side is
fastx.GetSeqsMap keyed by the FULL name (PARITY.md PFILE), the FASTQ side looks its record ID up."""
import re

_DNA = bytes.maketrans(b"acgtryswkmbdhvACGTRYSWKMBDHV", b"tgcayrswmkvhdbTGCAYRSWMKVHDB")
_RNA = bytes.maketrans(b"acguryswkmbdhvACGURYSWKMBDHV", b"ugcayrswmkvhdbUGCAYRSWMKVHDB")
COMPLEMENT = {"dna": _DNA, "rna": _RNA, "protein": None, "unlimit": None}


def read_fasta_map(text):
    """full name -> sequence: lines joined, `\\r` trimmed, a repeated name keeps the later sequence"""
    table, name = {}, None
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r")
        if line[:1] == b">":
            name = line[1:]
            table[name] = b""
        elif name is not None:
            table[name] += line
    return table


def fastq_records(data):
    """(head, seq, qual) of every record; sequences and qualities may span lines (helper.go:252-269)"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out, k = [], 0
    while k < len(lines):
        head = lines[k][1:]
        k += 1
        seq = b""
        while k < len(lines) and lines[k][:1] != b"+":
            seq += lines[k]
            k += 1
        k += 1  # the '+' line
        qual = b""
        while k < len(lines) and (len(qual) < len(seq) or (not seq and not qual and lines[k][:1] != b"@")):
            qual += lines[k]
            k += 1
            if not seq:
                break
        out.append((head, seq, qual))
    return out


def record_id(head, id_regexp=""):
    """parseHeadIDAndDesc (helper.go:329-369)"""
    if id_regexp in ("", "^(\\S+)\\s?"):
        for sep in (b" ", b"\t"):
            i = head.find(sep)
            if i > 0:
                return head[:i]
        return head
    m = re.search(id_regexp.encode(), head)
    return m.group(1) if m else head


def verdicts(shard, fasta, opts):
    """per record: (kind, id, seq slice, qual slice) with kind in plus / minus / absent / nohit"""
    table = read_fasta_map(fasta)
    comp = COMPLEMENT[opts.get("SeqType", "dna")]
    out = []
    for head, seq, qual in fastq_records(shard):
        rid = record_id(head, opts.get("IDRegexp", ""))
        if rid not in table:
            out.append(("absent", rid, b"", b""))
            continue
        fa = table[rid]
        i = seq.find(fa)
        if i >= 0:
            out.append(("plus", rid, seq[i:i + len(fa)], qual[i:i + len(fa)]))
            continue
        if not opts.get("OnlyPositiveStrand", False):
            rc = seq[::-1].translate(comp) if comp else seq[::-1]
            rq = qual[::-1]
            i = rc.find(fa)
            if i >= 0:
                out.append(("minus", rid, rc[i:i + len(fa)], rq[i:i + len(fa)]))
                continue
        out.append(("nohit", rid, b"", b""))
    return out


def fa2fq(shard, fasta, opts=None):
    return b"".join(b"@" + rid + b"\n" + s + b"\n+\n" + q + b"\n"
                    for kind, rid, s, q in verdicts(shard, fasta, opts or {}) if kind in ("plus", "minus"))
