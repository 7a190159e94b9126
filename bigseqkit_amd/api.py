"""Host-side mirror of the reference's driver library for the hot path.

Same entry points, argument meaning and error behaviour as
/root/reference/bigseqkit/{helper,stats}.go, but the dataflow
``MapPartitions(libSource("Stats")) -> Reduce(libSource("StatsReduce"))`` is a
sequence of C-ABI calls into libbsk.so (include/bsk.h) instead of IgnisHPC tasks.
"""
import ctypes as C
import itertools
import json
import os

from . import _lib
from ._lib import lib, check, BskError, FORMAT_FASTA, FORMAT_FASTQ
from .options import SeqKitStatsOptions, SeqKitSeqOptions, SeqKitGrepOptions, SeqKitSubseqOptions, SeqKitTranslateOptions, SeqKitRmDupOptions, SeqKitLocateOptions, SeqKitFq2FaOptions, SeqKitHeadOptions, SeqKitDuplicateOptions, SeqKitRenameOptions, SeqKitSortOptions, SeqKitFaidxOptions, SeqKitPairOptions, SeqKitCommonOptions, SeqKitConcatOptions, SeqKitReplaceOptions, SeqKitFa2FqOptions, SeqKitSampleOptions, SeqKitShuffleOptions, SeqKitHeadGenomeOptions


class SeqFrame:
    """What ``*api.IDataFrame[string]`` is to the reference: the records of one input,
    held as shards (partitions) of raw FASTA/FASTQ text that begin on a record.
    A shard is ``(buffer, nbytes, on_device)``; device buffers are anything with
    ``data_ptr()`` (a torch uint8 tensor), host buffers are bytes-like."""

    def __init__(self, fmt, shards):
        self.format = fmt
        self.shards = list(shards)

    @staticmethod
    def _ptr(buf):
        if hasattr(buf, "data_ptr"):
            return C.c_void_p(buf.data_ptr()), int(buf.numel()), bool(buf.is_cuda)
        mv = memoryview(buf)
        if mv.readonly:
            arr = (C.c_char * len(mv)).from_buffer_copy(mv)  # keeps a private copy alive
        else:
            arr = (C.c_char * len(mv)).from_buffer(mv)
        return C.cast(arr, C.c_void_p), len(mv), False, arr

    def partitions(self):
        for pid, buf in enumerate(self.shards):
            r = self._ptr(buf)
            yield pid, r[0], r[1], r[2], r  # keep r alive while the pointer is in use


def _read(path_or_bytes, fmt, min_partitions=1):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) or hasattr(path_or_bytes, "data_ptr"):
        data = path_or_bytes
    else:
        with open(os.fspath(path_or_bytes), "rb") as f:
            data = f.read()
    if hasattr(data, "data_ptr") or min_partitions <= 1:
        return SeqFrame(fmt, [data])
    # PlainFileN(path, minPartitions, delim) + ReadFixer: cut on record starts
    n = len(data)
    arr = (C.c_char * n).from_buffer_copy(data)
    cuts = [0]
    for k in range(1, min_partitions):
        out = C.c_size_t()
        check(lib.bsk_find_record_start(C.cast(arr, C.c_void_p), n, n * k // min_partitions, fmt, C.byref(out)))
        if out.value > cuts[-1]:
            cuts.append(out.value)
    cuts.append(n)
    return SeqFrame(fmt, [bytes(data[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])


def ReadFASTA(path, worker=None):
    """bigseqkit/helper.go:148-154"""
    return _read(path, FORMAT_FASTA)


def ReadFASTAN(path, minPartitions, worker=None):
    """bigseqkit/helper.go:156-162"""
    return _read(path, FORMAT_FASTA, minPartitions)


def ReadFASTQ(path, worker=None):
    """bigseqkit/helper.go:164-170"""
    return _read(path, FORMAT_FASTQ)


def ReadFASTQN(path, minPartitions, worker=None):
    """bigseqkit/helper.go:172-178"""
    return _read(path, FORMAT_FASTQ, minPartitions)


# ---- BGZF input (include/bsk.h "BGZF input"; PARITY.md BGZF)
def BgzfProbe(data):
    """0: not gzip, 1: BGZF, 2: gzip that is not BGZF -- from the first bytes of a file"""
    head = bytes(data[:12 + 65535])
    return int(lib.bsk_bgzf_probe(head, len(head)))


def _device_input(data, device):
    """(tensor or None to keep alive, pointer, bytes) of a compressed input on `device`"""
    import torch
    if hasattr(data, "data_ptr"):
        if not data.is_cuda:
            data = data.to("cuda:%d" % device)
        torch.cuda.synchronize(data.device)
        return data, C.c_void_p(data.data_ptr()), int(data.numel())
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:%d" % device) if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda:%d" % device)
    torch.cuda.synchronize(t.device)
    return t, C.c_void_p(t.data_ptr() if len(data) else 0), len(data)


def _adopt(d_text, n, device):
    """the library's buffer as a tensor of torch's own (one copy on the device), the library's freed"""
    import torch
    out = torch.empty(n, dtype=torch.uint8, device="cuda:%d" % device)
    try:
        if n:
            check(lib.bsk_device_copy(C.c_void_p(out.data_ptr()), d_text, n, 3))  # BSK_COPY_D2D
    finally:
        lib.bsk_device_free(d_text)
    return out


def _inflate(host, on_device, data, device, host_extra, device_extra):
    """the double call of a host inflate (size, then fill), or the device call and its buffer adopted.  host_extra: what the
    host entry point takes behind its output (threads, or chunk_bytes); device_extra: what the device's takes in front of it"""
    n_text = C.c_size_t()
    if device < 0:
        data = bytes(data)
        check(host(data, len(data), None, 0, C.byref(n_text), *host_extra))
        buf = C.create_string_buffer(max(1, n_text.value))
        check(host(data, len(data), buf, n_text.value, C.byref(n_text), *host_extra))
        return buf.raw[:n_text.value]
    keep, ptr, n = _device_input(data, device)
    d_text = C.c_void_p()
    check(on_device(ptr, n, device, *device_extra, C.byref(d_text), C.byref(n_text)))
    del keep
    return _adopt(d_text, n_text.value, device)


def BgzfInflate(data, device=0):
    """the text of a BGZF file: bytes or a CUDA uint8 tensor in, a CUDA uint8 tensor out, inflated on the device.
    device=-1: bytes in, bytes out, the same decoder on host threads"""
    return _inflate(lib.bsk_bgzf_inflate_host, lib.bsk_bgzf_inflate_device, data, device, (0,), ())   # (0: the default number of threads)


# ---- plain gzip input (include/bsk.h "plain gzip input"; PARITY.md GZIP)
def GzipInflate(data, device=0, chunk_bytes=0):
    """the text of a gzip file of any number of members: bytes or a CUDA uint8 tensor in, a CUDA uint8 tensor out, inflated on
    the device in speculative chunks of chunk_bytes (0: the library's choice).  device=-1: bytes in, bytes out, the same method
    with one host lane (chunk_bytes 0: one piece)"""
    return _inflate(lib.bsk_gzip_inflate_host, lib.bsk_gzip_inflate_device, data, device, (chunk_bytes,), (chunk_bytes,))


_PLAN_FIELDS = ("chunks", "with_candidate", "on_chain", "off_chain", "members", "text_bytes", "dropped_bytes", "chunk_bytes")


def GzipPlan():
    """the numbers of the last GzipInflate / gzip ReadSeqFile on this thread, as a dict: chunks, with_candidate (chunks in which
    a block start was found), on_chain (chunks that the true chain of blocks visits, the first included), off_chain (candidates
    that were dropped), members, text_bytes, dropped_bytes (decoded by chunks that were dropped), chunk_bytes"""
    out = (C.c_uint64 * 8)()
    lib.bsk_gzip_last_plan(out)
    return dict(zip(_PLAN_FIELDS, (int(v) for v in out)))


def BgzfBlocks(data, device=0):
    """the block index: [(offset in the file, size of the block, bytes it holds), ...]"""
    keep, ptr, n = _device_input(data, device)
    count = C.c_size_t()
    check(lib.bsk_bgzf_blocks_device(ptr, n, device, None, None, None, 0, C.byref(count)))
    k = count.value
    coff, csize, usize = (C.c_uint64 * max(1, k))(), (C.c_uint32 * max(1, k))(), (C.c_uint32 * max(1, k))()
    check(lib.bsk_bgzf_blocks_device(ptr, n, device, coff, csize, usize, k, C.byref(count)))
    del keep
    return [(int(coff[i]), int(csize[i]), int(usize[i])) for i in range(k)]


class BgzfReader:
    """the text of a BGZF file in record-aligned pieces (bsk_bgzf_reader_*): the file is never held whole, compressed or
    inflated.  Iterating gives (piece, voff_lo, voff_hi): the piece a CUDA uint8 tensor that VIEWS the reader's buffer --
    valid until the second piece after it, clone it to keep it -- or, with device=-1, bytes from the same reader on the
    host.  The offsets are BGZF virtual offsets; .piece(lo, hi) gives the bytes of a piece again on a later pass.
    0 for a size: 1 GiB of text, 1 MiB of lookahead, 256 MiB of compressed bytes.

        with BgzfReader("reads.fq.gz", FORMAT_FASTQ) as r:
            where = [(lo, hi) for _, lo, hi in r]
            again = r.piece(*where[0])
    """

    def __init__(self, path, fmt, device=0, piece_text_bytes=0, lookahead_bytes=0, comp_chunk_bytes=0):
        self.device = device
        self._f = open(os.fspath(path), "rb")
        self._r = C.c_void_p()
        self._done = False
        try:
            check(lib.bsk_bgzf_reader_open(self._f.fileno(), device, fmt, piece_text_bytes, lookahead_bytes, comp_chunk_bytes, C.byref(self._r)))
        except Exception:
            self._f.close()
            raise

    def close(self):
        if self._r:
            lib.bsk_bgzf_reader_close(self._r)
            self._r = C.c_void_p()
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _wrap(self, ptr, n):
        if self.device < 0:
            return C.string_at(ptr, n) if n else b""
        return _view(ptr.value, n, self.device)

    def seek(self, voff):
        check(lib.bsk_bgzf_reader_seek(self._r, voff))
        self._done = False

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        ptr, n, lo, hi, last = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib.bsk_bgzf_reader_next(self._r, C.byref(ptr), C.byref(n), C.byref(lo), C.byref(hi), C.byref(last)))
        self._done = bool(last.value)
        return self._wrap(ptr, n.value), lo.value, hi.value

    def piece(self, voff_lo, voff_hi):
        ptr, n = C.c_void_p(), C.c_size_t()
        check(lib.bsk_bgzf_reader_piece(self._r, voff_lo, voff_hi, C.byref(ptr), C.byref(n)))
        return self._wrap(ptr, n.value)


_READER_INFO_FIELDS = ("segments", "access_points", "doublings", "dropped_chunks", "members", "text_bytes", "peak_bytes", "chunk_bytes")


class GzipReader:
    """the text of a plain gzip file of any size in record-aligned pieces (bsk_gzip_reader_*): a segment of the file is held at
    a time, never the file or its text.  Iterating gives (piece, text_lo, text_hi) and checks every member's CRC32 and ISIZE;
    the piece a CUDA uint8 tensor that VIEWS the reader's buffer -- valid until the second piece after it, clone it to keep
    it -- or, with device=-1, bytes from the same reader on the host.  The offsets are offsets of the text;
    .piece(lo, hi) gives the bytes of a piece again on a later pass (the reader re-enters at the segment start in front of lo).
    0 for a size: 1 GiB of text, 1 MiB of lookahead, 64 MiB of compressed bytes, the library's chunk rule.

        with GzipReader("reads.fq.gz", FORMAT_FASTQ) as r:
            where = [(lo, hi) for _, lo, hi in r]
            again = r.piece(*where[0])
    """

    def __init__(self, path, fmt, device=0, piece_text_bytes=0, lookahead_bytes=0, segment_bytes=0, chunk_bytes=0):
        self.device = device
        self._f = open(os.fspath(path), "rb")
        self._r = C.c_void_p()
        self._done = False
        try:
            check(lib.bsk_gzip_reader_open(self._f.fileno(), device, fmt, piece_text_bytes, lookahead_bytes, segment_bytes, chunk_bytes, C.byref(self._r)))
        except Exception:
            self._f.close()
            raise

    def close(self):
        if self._r:
            lib.bsk_gzip_reader_close(self._r)
            self._r = C.c_void_p()
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _wrap(self, ptr, n):
        if self.device < 0:
            return C.string_at(ptr, n) if n else b""
        return _view(ptr.value, n, self.device)

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        ptr, n, lo, hi, last = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib.bsk_gzip_reader_next(self._r, C.byref(ptr), C.byref(n), C.byref(lo), C.byref(hi), C.byref(last)))
        self._done = bool(last.value)
        return self._wrap(ptr, n.value), lo.value, hi.value

    def piece(self, text_lo, text_hi):
        ptr, n = C.c_void_p(), C.c_size_t()
        check(lib.bsk_gzip_reader_piece(self._r, text_lo, text_hi, C.byref(ptr), C.byref(n)))
        return self._wrap(ptr, n.value)

    def info(self):
        out = (C.c_uint64 * 8)()
        check(lib.bsk_gzip_reader_info(self._r, out))
        return dict(zip(_READER_INFO_FIELDS, (int(v) for v in out)))


class _Foreign:
    """n bytes of device memory that the library owns, for torch to look at (__cuda_array_interface__)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}


def _view(ptr, n, device):
    import torch
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda:%d" % device)
    return torch.as_tensor(_Foreign(ptr, n), device="cuda:%d" % device)


# ---- BGZF output (include/bsk.h "BGZF output"; PARITY.md BGZFW)
def BgzfDeflateHost(data, block_bytes=0, eof=True, threads=0):
    """the BGZF file that holds `data` (bytes), encoded on host threads: the bytes BgzfDeflate gives"""
    data = bytes(data)
    cap = int(lib.bsk_bgzf_deflate_bound(len(data), block_bytes))
    buf = C.create_string_buffer(max(1, cap))
    n_out = C.c_size_t()
    check(lib.bsk_bgzf_deflate_host(data, len(data), block_bytes, 1 if eof else 0, buf, cap, C.byref(n_out), threads))
    return buf.raw[:n_out.value]


def BgzfDeflate(data, device=0, block_bytes=0, eof=True):
    """the BGZF file that holds `data`: bytes or a CUDA uint8 tensor in, bytes out, one block per wavefront on the device (only
    the compressed bytes come back).  block_bytes: the text of a block, 0 = 65 280.  device=-1: BgzfDeflateHost"""
    if device < 0:
        return BgzfDeflateHost(data, block_bytes, eof)
    keep, ptr, n = _device_input(data, device)
    d_comp, n_comp = C.c_void_p(), C.c_size_t()
    check(lib.bsk_bgzf_deflate_device(ptr, n, device, block_bytes, 1 if eof else 0, C.byref(d_comp), C.byref(n_comp)))
    del keep
    buf = C.create_string_buffer(max(1, n_comp.value))
    try:
        if n_comp.value:
            check(lib.bsk_device_copy(buf, d_comp, n_comp.value, 2))  # BSK_COPY_D2H
    finally:
        lib.bsk_device_free(d_comp)
    return buf.raw[:n_comp.value]


def WriteSeqFile(path, text_or_result, device=0):
    """the counterpart of ReadSeqFile: the text -- bytes, a uint8 tensor, or a SeqFrame, whose shards follow each other -- goes
    to `path`.  A path that ends in .gz / .bgz gets BGZF (text on the device is compressed there, bytes on host threads; the
    pieces end with ONE EOF block), anything else the plain text.  Returns the bytes written"""
    parts = text_or_result.shards if isinstance(text_or_result, SeqFrame) else [text_or_result]
    packed = os.fspath(path).lower().endswith((".gz", ".bgz"))
    total = 0
    with open(os.fspath(path), "wb") as f:
        for part in parts:
            on_device = hasattr(part, "data_ptr") and part.is_cuda
            if hasattr(part, "data_ptr") and not on_device:   # (a tensor in host memory: its bytes, not its elements one by one)
                part = part.numpy().tobytes()
            if packed:
                piece = BgzfDeflate(part, part.device.index if on_device else -1, 0, False)
            elif on_device:
                piece = bytes(part.cpu().numpy().tobytes())
            else:
                piece = bytes(part)
            f.write(piece)
            total += len(piece)
        if packed:
            tail = BgzfDeflateHost(b"", 0, True)   # the EOF block
            f.write(tail)
            total += len(tail)
    return total


def _format_of(path, first):
    """the format of a file: its first TEXT byte, else the suffix under a trailing .gz / .bgz"""
    if first == b">":
        return FORMAT_FASTA
    if first == b"@":
        return FORMAT_FASTQ
    name = os.fspath(path).lower()
    for z in (".gz", ".bgz"):
        if name.endswith(z):
            name = name[:-len(z)]
    if name.endswith((".fa", ".fasta", ".fna", ".faa")):
        return FORMAT_FASTA
    if name.endswith((".fq", ".fastq")):
        return FORMAT_FASTQ
    raise BskError(_lib.BSK_ERR_FORMAT, "%s must be fasta or fastq" % os.fspath(path))


def ReadSeqFile(path, device=0, gzip=False):
    """a FASTA / FASTQ file, plain or BGZF, as a SeqFrame over one shard.  A BGZF file crosses to the device compressed and is
    inflated there (bsk_bgzf_load); a plain one is read as ReadFASTA / ReadFASTQ read it.  gzip that is not BGZF is refused,
    unless gzip=True: then it crosses compressed too and is inflated in speculative chunks (bsk_gzip_load)"""
    with open(os.fspath(path), "rb") as f:
        head = f.read(12 + 65535)
        kind = BgzfProbe(head)
        if kind == 2 and not gzip:
            raise BskError(_lib.BSK_ERR_UNSUPPORTED, "%s is gzip but not BGZF: one gzip stream cannot be cut into independent blocks; recompress it with bgzip" % os.fspath(path))
        if kind == 0:
            return SeqFrame(_format_of(path, head[:1]), [head + f.read()])
        d_text, n_text = C.c_void_p(), C.c_size_t()
        load, extra = (lib.bsk_gzip_load, (0,)) if kind == 2 else (lib.bsk_bgzf_load, ())   # (gzip: chunk_bytes 0, the library's choice)
        check(load(f.fileno(), device, 0, *extra, C.byref(d_text), C.byref(n_text)))
    t = _adopt(d_text, n_text.value, device)
    return SeqFrame(_format_of(path, bytes(t[:1].cpu().numpy().tobytes())), [t])


# ---- a BGZF file under several workers (include/bsk.h "BGZF under several workers"; PARITY.md BGZF "workers")
def BgzfCutPoints(path, format, world):
    """where `world` workers cut the BGZF file `path`: world + 1 virtual offsets, worker k owns the text [v[k], v[k + 1]).
    Found on the host from the file around size * k / world (bsk_bgzf_cut_points); no device is touched"""
    voffs = (C.c_uint64 * (world + 1))()
    with open(os.fspath(path), "rb") as f:
        check(lib.bsk_bgzf_cut_points(f.fileno(), format, world, voffs))
    return [int(v) for v in voffs]


def BgzfShardLoad(path, voff_lo, voff_hi, device=0):
    """the text [voff_lo, voff_hi) of the BGZF file `path` as a SeqFrame over one shard on `device`: only the blocks of the range
    cross to the device, where they are inflated (bsk_bgzf_shard_load).  The offsets are BgzfCutPoints'.  An empty shard takes
    its format from the file's name"""
    d_text, n_text = C.c_void_p(), C.c_size_t()
    with open(os.fspath(path), "rb") as f:
        check(lib.bsk_bgzf_shard_load(f.fileno(), voff_lo, voff_hi, device, 0, C.byref(d_text), C.byref(n_text)))
    t = _adopt(d_text, n_text.value, device)
    return SeqFrame(_format_of(path, bytes(t[:1].cpu().numpy().tobytes())), [t])


class Operator:
    """One plugin operator between Before() and After() (bsk_create .. bsk_destroy)."""

    def __init__(self, name, opts_json, device=0):
        self.ctx = C.c_void_p()
        if isinstance(opts_json, str):
            opts_json = opts_json.encode()
        check(lib.bsk_create(name.encode(), opts_json, device, C.byref(self.ctx)))

    def close(self):
        if self.ctx:
            lib.bsk_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def opts_json(self):
        return lib.bsk_opts_json(self.ctx).decode()


def _collect_map(op, d_vec=None):
    cap = 1024
    while True:
        n = C.c_size_t()
        keys = (C.c_int64 * cap)()
        vals = (C.c_int64 * cap)()
        rc = lib.bsk_stats_collect(op.ctx, d_vec, keys, vals, cap, C.byref(n))
        if rc == _lib.BSK_ERR_CAPACITY and n.value > cap:
            cap = n.value
            continue
        check(rc, op.ctx)
        return dict(zip(keys[:n.value], vals[:n.value]))


def stats_map(input, o=None, device=0, stream=None):
    """MapPartitions(Stats) + Reduce(StatsReduce) (bigseqkit/stats.go:81-94): the merged
    map[int64]int64.  Returns (map, operator) -- the operator carries the first record
    the driver needs for the type column."""
    o = o or SeqKitStatsOptions()
    op = Operator("Stats", o.to_json(), device)
    try:
        for pid, ptr, n, on_dev, keep in input.partitions():
            check(lib.bsk_stats_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, None, stream), op.ctx)
        return _collect_map(op), op
    except Exception:
        op.close()
        raise


def _finalize(op, m):
    ks = sorted(m)
    keys = (C.c_int64 * len(ks))(*ks)
    vals = (C.c_int64 * len(ks))(*[m[k] for k in ks])
    info = _lib.StatInfo()
    check(lib.bsk_stats_finalize(op.ctx, keys, vals, len(ks), C.byref(info)), op.ctx)
    return info


def Stats(name, format, input, o=None, device=0):
    """bigseqkit/stats.go:75-166 -> StatInfo"""
    m, op = stats_map(input, o, device)
    with op:
        return _finalize(op, m)


def StatsString(name, format, input, o=None, device=0):
    """bigseqkit/stats.go:168-288"""
    m, op = stats_map(input, o, device)
    with op:
        info = _finalize(op, m)
        buf = C.create_string_buffer(1 << 16)
        check(lib.bsk_stats_string(op.ctx, name.encode(), format.encode(), C.byref(info), buf, len(buf)), op.ctx)
        return buf.value.decode()


def _out_bytes(op, out):
    """the text of a bsk_out, copied to the host"""
    buf = C.create_string_buffer(max(1, out.len))
    check(lib.bsk_out_to_host(op.ctx, C.byref(out), buf, out.len), op.ctx)
    return buf.raw[:out.len]


_BUCKET_BINS = 4096   # the fine bins of shuffle, sort and rmdup in buckets: bsk_shuffle_plan plans all three


# The key-bucket family (shuffle, sort, rmdup, rename, common, pair and its order phase, concat): a command's entry points are
# bsk_<prefix>_<step> with the same signatures (_lib.py), so one helper per kind of step serves all of them; the public
# functions further down are one-liners over these.
def _bsk(prefix, step):
    return getattr(lib, "bsk_%s_%s" % (prefix, step))


def _count_pass(fn, op, input, *extra, counts=None, first=0):
    """fn(ctx, shard ..., first_record, *extra, stream, &n_records) over the shards of `input`, in order, every shard told where
    it starts -- the first at global record `first`, the next behind the records the pass counted, or behind counts[j] where
    the caller knows them: the record count of every shard"""
    got = []
    for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), itertools.repeat(None) if counts is None else counts):
        k = C.c_uint64()
        check(fn(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, *extra, None, C.byref(k)), op.ctx)
        got.append(k.value)
        first += k.value if cnt is None else cnt
    return got


def _hist_get(prefix, op):
    """bsk_<prefix>_hist_get: (bytes[4096], records[4096])"""
    b, r = (C.c_uint64 * _BUCKET_BINS)(), (C.c_uint64 * _BUCKET_BINS)()
    check(_bsk(prefix, "hist_get")(op.ctx, b, r), op.ctx)
    return list(b), list(r)


def _hist_reset(prefix, op):
    check(_bsk(prefix, "hist_reset")(op.ctx), op.ctx)


def _bucket_adds(prefix, op, input, counts, lo_bin, hi_bin, first=0):
    """bsk_<prefix>_bucket_begin, then _bucket_add of every shard of `input`, in order, the first at global record `first`"""
    check(_bsk(prefix, "bucket_begin")(op.ctx, lo_bin, hi_bin), op.ctx)
    for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), counts):
        check(_bsk(prefix, "bucket_add")(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None), op.ctx)
        first += cnt


def _counted_bucket(prefix, op, input, counts, lo_bin, hi_bin):
    """_bucket_adds, then bsk_<prefix>_bucket_finish: its two counters"""
    _bucket_adds(prefix, op, input, counts, lo_bin, hi_bin)
    a, b = C.c_uint64(), C.c_uint64()
    check(_bsk(prefix, "bucket_finish")(op.ctx, None, C.byref(a), C.byref(b)), op.ctx)
    return a.value, b.value


def _out_bucket(prefix, op, input, counts, lo_bin, hi_bin, first=0):
    """_bucket_adds, then bsk_<prefix>_bucket_finish: the bytes of its bsk_out"""
    _bucket_adds(prefix, op, input, counts, lo_bin, hi_bin, first)
    out = _lib.Out()
    check(_bsk(prefix, "bucket_finish")(op.ctx, None, C.byref(out)), op.ctx)
    return _out_bytes(op, out)


def _emit_pass(fn, op, input, counts, first=0):
    """fn(ctx, shard ..., first_record, stream, &out) over the shards of `input`, in order, the first at global record `first`:
    the outputs, joined"""
    chunks = []
    for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), counts):
        out = _lib.Out()
        check(fn(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None, C.byref(out)), op.ctx)
        chunks.append(_out_bytes(op, out))
        first += cnt
    return b"".join(chunks)


def _run_records(op_name, run_fn, input, o, device=0, stream=None, finish=None):
    """MapPartitions(libSource(op_name)) over the shards of `input`: the concatenated
    FileStore bytes (element + newline per output record) and the number of elements."""
    chunks, nrec = [], 0
    with Operator(op_name, o.to_json(), device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            out = _lib.Out()
            check(run_fn(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, stream, C.byref(out)), op.ctx)
            chunks.append(_out_bytes(op, out))
            nrec += out.records
        if finish is not None:  # After() with an error return
            check(finish(op.ctx), op.ctx)
    return b"".join(chunks), nrec


def _one_shard(input):
    """The operators whose result depends on ALL records (rmdup, rename, sort, grep --delete-matched: GroupByKey /
    SortByKey / Reduce over the whole dataframe in the reference) see the input as ONE shard: the shards of `input`
    back to back, a newline added where a shard lacks the final one (what cli/bigseqkit.cpp does with several input
    files).  Across ranks the exchange of dist.py takes this place."""
    if len(input.shards) <= 1:
        return input
    if all(hasattr(b, "data_ptr") for b in input.shards):
        both, _ = _join_files(list(input.shards))
        return SeqFrame(input.format, [both])
    if any(hasattr(b, "data_ptr") for b in input.shards):
        raise ValueError("a SeqFrame must hold either host or device shards, not both")
    parts = []
    for b in input.shards:
        b = bytes(b)
        parts.append(b if (not b or b.endswith(b"\n")) else b + b"\n")
    return SeqFrame(input.format, [b"".join(parts)])


def Seq(input, o=None, device=0):
    """bigseqkit/seq.go:157-170 -- returns the bytes StoreFASTX would write"""
    return _run_records("SeqTransform", lib.bsk_seq_run, input, o or SeqKitSeqOptions(), device)[0]


def Grep(input, o, device=0):
    """bigseqkit/grep.go:130-159 (Count forced off, :136-137)"""
    o._v["Count"] = False
    if o._v.get("DeleteMatched"):  # the driver keeps the lowest partition per pattern (bigseqkit/grep.go:144-156): global
        input = _one_shard(input)
    return _run_records("Grep", lib.bsk_grep_run, input, o, device)[0]


def GrepCount(input, o, device=0):
    """bigseqkit/grep.go:161-180: per-partition counts summed (GrepReduceCount)"""
    o._v["Count"] = True
    total = 0
    with Operator("Grep", o.to_json(), device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            out = _lib.Out()
            check(lib.bsk_grep_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, None, C.byref(out)), op.ctx)
            cnt = C.c_uint64()
            check(lib.bsk_grep_last_count(op.ctx, C.byref(cnt)), op.ctx)
            total += cnt.value
    return total


def Subseq(input, o, device=0):
    """bigseqkit/subseq.go:86-100"""
    return _run_records("SubseqTransform", lib.bsk_subseq_run, input, o, device)[0]


def Locate(input, o, device=0):
    """bigseqkit/locate.go:122-134 (MapPartitionsWithIndex: partition 0 carries the header row)"""
    return _run_records("Locate", lib.bsk_locate_run, input, o, device)[0]


def Translate(input, o=None, device=0):
    """bigseqkit/translate.go:87-100"""
    return _run_records("Translate", lib.bsk_translate_run, input, o or SeqKitTranslateOptions(), device)[0]


def RmDup(input, o=None, device=0):
    """bigseqkit/rmdup.go:70-108 (GroupByKey, :97: duplicates are global -- several shards are joined into one)"""
    return _run_records("RmDup", lib.bsk_rmdup_run, _one_shard(input), o or SeqKitRmDupOptions(), device,
                        finish=lib.bsk_rmdup_finish)[0]


def Fq2Fa(input, o=None, device=0):
    """bigseqkit/fq2fa.go:25-37"""
    return _run_records("Fq2Fa", lib.bsk_fq2fa_run, input, o or SeqKitFq2FaOptions(), device)[0]


def Duplicate(input, o=None, device=0):
    """bigseqkit/duplicate.go:31-43 (Flatmap: the copies of a record are adjacent)"""
    return _run_records("Duplicate", lib.bsk_duplicate_run, input, o or SeqKitDuplicateOptions(), device)[0]


def Rename(input, o=None, device=0):
    """bigseqkit/rename.go:34-60 (ordinals count over the whole dataframe: several shards are joined, like RmDup)"""
    return _run_records("Rename", lib.bsk_rename_run, _one_shard(input), o or SeqKitRenameOptions(), device)[0]


def Replace(input, o, device=0):
    """bigseqkit/replace.go:39-60 (MapPartitions: {nr} counts the records of each shard from 1)"""
    return _run_records("Replace", lib.bsk_replace_run, input, o or SeqKitReplaceOptions(), device)[0]


def Fa2Fq(input, o, device=0):
    """bigseqkit/fa2fq.go:42-56 (MapPartitions; every shard is joined against the same FASTA table)"""
    return _run_records("Fa2Fq", lib.bsk_fa2fq_run, input, o or SeqKitFa2FqOptions(), device)[0]


def Sort(input, o=None, device=0):
    """bigseqkit/sort.go:91-147 (SortByKey over the whole dataframe: several shards are joined)"""
    return _run_records("Sort", lib.bsk_sort_run, _one_shard(input), o or SeqKitSortOptions(), device)[0]


def Faidx(input, o=None, device=0):
    """bigseqkit/faidx.go:61-95 (index rows only): the FaidxOffset pass is the running sum of the shard sizes"""
    chunks, base = [], 0
    with Operator("Faidx", (o or SeqKitFaidxOptions()).to_json(), device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            out = _lib.Out()
            check(lib.bsk_faidx_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, base, None, C.byref(out)), op.ctx)
            chunks.append(_out_bytes(op, out))
            base += n
    return b"".join(chunks)


def Pair(inputA, inputB, o=None, device=0):
    """bigseqkit/pair.go:68-100 -> (paired.1, paired.2, unpaired.1, unpaired.2) as the bytes SaveAsTextFile would write.
    Both inputs are one device-resident shard each; they are joined (file 1, then file 2) for the one call."""
    import torch
    a, b = inputA.shards[0], inputB.shards[0]
    if not (hasattr(a, "data_ptr") and hasattr(b, "data_ptr")):
        raise ValueError("Pair: both inputs must be device tensors")
    parts = [a]
    if a.numel() and int(a[-1]) != 10:
        parts.append(torch.tensor([10], dtype=torch.uint8, device=a.device))
    n_first = sum(p.numel() for p in parts)
    both = torch.cat(parts + [b]) if b.numel() or len(parts) > 1 else a
    outs = (_lib.Out * 4)()
    res = []
    with Operator("Pair", (o or SeqKitPairOptions()).to_json(), device) as op:
        check(lib.bsk_pair_run(op.ctx, C.c_void_p(both.data_ptr()) if both.numel() else None, both.numel(), n_first, 1,
                               inputA.format, None, outs), op.ctx)
        for k in range(4):
            buf = C.create_string_buffer(max(1, outs[k].len))
            check(lib.bsk_out_to_host(op.ctx, C.byref(outs[k]), buf, outs[k].len), op.ctx)
            res.append(buf.raw[:outs[k].len])
    return tuple(res)


def _join_files(tensors):
    """device tensors back to back, a newline added to a file that lacks the final one -> (tensor, [end offsets])"""
    import torch
    parts, ends, at = [], [], 0
    for t in tensors:
        parts.append(t)
        at += t.numel()
        if t.numel() and int(t[-1]) != 10:
            parts.append(torch.tensor([10], dtype=torch.uint8, device=t.device))
            at += 1
        ends.append(at)
    return (torch.cat(parts) if len(parts) > 1 else parts[0]), ends


def Common(inputA, inputB, o=None, *inputN, device=0):
    """bigseqkit/common.go:68-109 -> the records of inputA common to all inputs (one device-resident shard each)"""
    frames = [inputA, inputB, *inputN]
    both, ends = _join_files([f.shards[0] for f in frames])
    arr = (C.c_uint64 * len(ends))(*ends)
    out = _lib.Out()
    with Operator("Common", (o or SeqKitCommonOptions()).to_json(), device) as op:
        check(lib.bsk_common_run(op.ctx, C.c_void_p(both.data_ptr()) if both.numel() else None, both.numel(), arr, len(ends), 1,
                                 inputA.format, None, C.byref(out)), op.ctx)
        return _out_bytes(op, out)


def Concat(inputA, inputB, o=None, device=0):
    """bigseqkit/concat.go:53-90 (one device-resident shard per input)"""
    both, ends = _join_files([inputA.shards[0], inputB.shards[0]])
    out = _lib.Out()
    with Operator("Concat", (o or SeqKitConcatOptions()).to_json(), device) as op:
        check(lib.bsk_concat_run(op.ctx, C.c_void_p(both.data_ptr()) if both.numel() else None, both.numel(), ends[0], 1,
                                 inputA.format, None, C.byref(out)), op.ctx)
        return _out_bytes(op, out)


def FaidxQuery(input, o, device=0):
    """the `queries` dataframe of bigseqkit/faidx.go:96-106 (Regions / RegionFile of the options)"""
    return _run_records("Faidx", lib.bsk_faidx_query_run, input, o, device)[0]


class FaidxFetchPlan:
    """The plan of `faidx -d` (bsk_faidx_fetch_plan; PARITY.md FAIX): the rows of an index `fai` (bytes), the regions of the
    options `o` and the size of the sequence file -> hits in row order, and batches with the spans of the file they read.
    Host only: device=-1 needs no GPU and nothing is read.  `op` is the Faidx operator the plan belongs to."""

    def __init__(self, fai, o, file_size, device=-1, format=-1, budget=0):
        self.op = Operator("Faidx", o.to_json(), device)
        self.ptr = C.c_void_p()
        try:
            check(lib.bsk_faidx_fetch_plan(self.op.ctx, fai, len(fai), file_size, format, budget, C.byref(self.ptr)), self.op.ctx)
            v = (C.c_uint64 * 8)()
            check(lib.bsk_faidx_fetch_plan_counts(self.ptr, v))
            self.rows, nh, nb, fq, self.T, self.read_bytes, self.out_bytes, self.alphabet_bytes = [int(x) for x in v]
            self.fastq = bool(fq)
            w = (C.c_uint64 * (8 * max(1, nh)))()
            check(lib.bsk_faidx_fetch_plan_hits(self.ptr, w, nh))
            self.hits = []
            for k in range(nh):
                row, p0, p1, minus, lo, hi, probe, out_len = [int(x) for x in w[8 * k:8 * k + 8]]
                n = C.c_size_t()
                buf = C.create_string_buffer(65536)
                check(lib.bsk_faidx_fetch_plan_header(self.ptr, k, buf, len(buf), C.byref(n)))
                self.hits.append(dict(row=row, p0=p0, p1=p1, minus=bool(minus), lines=(lo, hi), probe=probe, out_len=out_len,
                                      header=buf.raw[:n.value]))
            self.batches = []
            for b in range(nb):
                head, n = (C.c_uint64 * 4)(), C.c_size_t()
                lib.bsk_faidx_fetch_plan_batch(self.ptr, b, head, None, 0, C.byref(n))
                sp = (C.c_uint64 * (2 * max(1, n.value)))()
                check(lib.bsk_faidx_fetch_plan_batch(self.ptr, b, head, sp, n.value, C.byref(n)))
                self.batches.append(dict(hits=(int(head[0]), int(head[1])), read_bytes=int(head[2]), out_bytes=int(head[3]),
                                         spans=[(int(sp[2 * k]), int(sp[2 * k + 1])) for k in range(n.value)]))
        except Exception:
            self.close()
            raise

    def close(self):
        if self.ptr:
            lib.bsk_faidx_fetch_plan_free(self.ptr)
            self.ptr = C.c_void_p()
        self.op.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        """bsk_faidx_fetch_info: what the last fetch of the calling thread did"""
        v = (C.c_uint64 * 8)()
        check(lib.bsk_faidx_fetch_info(self.op.ctx, v), self.op.ctx)
        return dict(hits=int(v[0]), spans=int(v[1]), bytes_read=int(v[2]), blocks_inflated=int(v[3]), T=int(v[4]), tiles=int(v[5]),
                    bytes_written=int(v[6]))


def BgzfGzi(path):
    """The block table of a BGZF file by a header walk (bsk_bgzf_gzi_build: BSIZE and ISIZE of every block, no inflate) ->
    (the image of FILE.gzi as htslib writes it, bytes of text)"""
    import os
    fd = os.open(path, os.O_RDONLY)
    try:
        n, text = C.c_size_t(), C.c_uint64()
        lib.bsk_bgzf_gzi_build(fd, None, 0, C.byref(n), C.byref(text))
        buf = C.create_string_buffer(max(1, n.value))
        check(lib.bsk_bgzf_gzi_build(fd, buf, n.value, C.byref(n), C.byref(text)))
        return buf.raw[:n.value], text.value
    finally:
        os.close(fd)


def FaidxFetch(path, fai, o, device=0, gzi=None, host=False, budget=0, info=None):
    """`faidx -d`: the regions of the options `o` fetched from the sequence file `path` through the index rows `fai` (bytes,
    as Faidx wrote them for that file): the bytes of FaidxQuery on the whole file, the file never loaded whole.  gzi: `path`
    is a BGZF file and gzi the image of its block table (BgzfGzi(path)[0], or the bytes of FILE.gzi); the rows' offsets are
    text offsets.  host=True: the same source on one host lane (bsk_faidx_fetch_host; device=-1 then needs no GPU).  info: a
    dict that takes the sums of bsk_faidx_fetch_info over the batches."""
    import os
    fd = os.open(path, os.O_RDONLY)
    try:
        size = os.fstat(fd).st_size
        if gzi is not None:
            t = C.c_uint64()
            check(lib.bsk_bgzf_gzi_text_size(fd, gzi, len(gzi), C.byref(t)))
            size = t.value
        glen = len(gzi) if gzi is not None else 0
        chunks = []
        with FaidxFetchPlan(fai, o, size, device, -1, budget) as plan:
            for b in range(len(plan.batches)):
                if host:
                    n = C.c_size_t()
                    buf = C.create_string_buffer(max(1, plan.batches[b]["out_bytes"]))
                    check(lib.bsk_faidx_fetch_host(plan.op.ctx, fd, gzi, glen, plan.ptr, b, buf, len(buf), C.byref(n)), plan.op.ctx)
                    chunks.append(buf.raw[:n.value])
                else:
                    out = _lib.Out()
                    check(lib.bsk_faidx_fetch_run(plan.op.ctx, fd, gzi, glen, plan.ptr, b, 0, None, C.byref(out)), plan.op.ctx)
                    chunks.append(_out_bytes(plan.op, out))
                if info is not None:
                    for k, v in plan.info().items():
                        info[k] = v if k == "T" else info.get(k, 0) + v
        return b"".join(chunks)
    finally:
        os.close(fd)


def Count(input, device=0):
    """input.Count(): records per shard (the record table of every shard is built once)"""
    counts = []
    with Operator("SeqTransform", "{}", device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            nrec = C.c_uint64()
            check(lib.bsk_index_build(op.ctx, ptr, n, 1 if on_dev else 0, input.format, None, C.byref(nrec)), op.ctx)
            counts.append(nrec.value)
    return counts


def _range(op_name, input, o, device):
    """bigseqkit/range.go:36-103: MapWithIndex(RangePrepare) + Filter(RangeFilter); the index of a record is its
    position in the whole input, so every shard is told where it starts.  The counts cost one index pass per shard,
    which is what IgnisHPC's MapWithIndex (and input.Count() for negative positions) also pay."""
    chunks = []
    with Operator(op_name, o.to_json(), device) as op:
        counts = Count(input, device) if len(input.shards) > 1 else [0]
        needs = C.c_int()
        check(lib.bsk_range_needs_count(op.ctx, C.byref(needs)), op.ctx)
        if needs.value:
            if len(input.shards) == 1:
                counts = Count(input, device)
            check(lib.bsk_range_set_count(op.ctx, sum(counts)), op.ctx)
        first = 0
        for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), counts):
            out = _lib.Out()
            check(lib.bsk_range_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None, C.byref(out)), op.ctx)
            chunks.append(_out_bytes(op, out))
            first += cnt
    return b"".join(chunks)


def Range(input, o, device=0):
    """bigseqkit/range.go:36-103"""
    return _range("Range", input, o, device)


def Head(input, o=None, device=0):
    """bigseqkit/head.go:34-44: Range("1:N")"""
    return _range("Head", input, o or SeqKitHeadOptions(), device)


def Sample(input, o, device=0):
    """bigseqkit/sample.go:48-76: the verdict on a record depends on (Seed, its index in the whole input) alone, so every
    shard is told where it starts, as in Range; Count() only for Number > 0 or several shards."""
    chunks = []
    with Operator("Sample", o.to_json(), device) as op:
        counts = Count(input, device) if len(input.shards) > 1 else [0]
        needs = C.c_int()
        check(lib.bsk_sample_needs_count(op.ctx, C.byref(needs)), op.ctx)
        if needs.value:
            if len(input.shards) == 1:
                counts = Count(input, device)
            check(lib.bsk_sample_set_count(op.ctx, sum(counts)), op.ctx)
        first = 0
        for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), counts):
            out = _lib.Out()
            check(lib.bsk_sample_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None, C.byref(out)), op.ctx)
            chunks.append(_out_bytes(op, out))
            first += cnt
    return b"".join(chunks)


def Shuffle(input, o=None, device=0):
    """bigseqkit/shuffle.go:33-46 (PARITY SHUF): the records in ascending order of their draws; global, several shards are joined"""
    return _run_records("Shuffle", lib.bsk_shuffle_run, _one_shard(input), o or SeqKitShuffleOptions(), device)[0]


SHUFFLE_BINS = _BUCKET_BINS


def ShuffleHistRun(op, input):
    """bsk_shuffle_hist_run over the shards of `input`, in order: the record count of every shard (the histogram accumulates
    in the operator's context)"""
    return _count_pass(lib.bsk_shuffle_hist_run, op, input)


def ShuffleHistGet(op):
    """bsk_shuffle_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("shuffle", op)


def ShuffleHistReset(op):
    """bsk_shuffle_hist_reset: the context is about to see another input"""
    _hist_reset("shuffle", op)


def ShufflePlan(hist_bytes, budget_bytes):
    """bsk_shuffle_plan (no device): bounds[b] = first fine bin of bucket b, bounds[-1] = 4096"""
    h = (C.c_uint64 * SHUFFLE_BINS)(*hist_bytes)
    bounds = (C.c_uint64 * (SHUFFLE_BINS + 1))()
    nb = C.c_int()
    check(lib.bsk_shuffle_plan(h, budget_bytes, bounds, C.byref(nb)))
    return list(bounds[:nb.value + 1])


def ShuffleBucket(op, input, counts, lo_bin, hi_bin):
    """bsk_shuffle_bucket_begin / _add over the shards of `input` / _finish: the bytes of the bucket [lo_bin, hi_bin)"""
    return _out_bucket("shuffle", op, input, counts, lo_bin, hi_bin)


def ShuffleBuckets(input, o=None, budget_bytes=1 << 30, device=0):
    """Shuffle of an input of any size on one device (PARITY SHUF): the histogram of the draws over all shards, the plan of
    buckets of at most `budget_bytes`, then one collect sequence per bucket; the same bytes as Shuffle.  The input is read
    once plus once per bucket."""
    with Operator("Shuffle", (o or SeqKitShuffleOptions()).to_json(), device) as op:
        counts = ShuffleHistRun(op, input)
        bounds = ShufflePlan(ShuffleHistGet(op)[0], budget_bytes)
        return b"".join(ShuffleBucket(op, input, counts, lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:]))


SORT_BINS = _BUCKET_BINS
SORT_SAMPLES_PER_BIN = 32   # a starting value from sample-sort practice, not a measurement


def _pack_strings(strings):
    offs = (C.c_uint64 * (len(strings) + 1))()
    at = 0
    for j, s in enumerate(strings):
        at += len(s)
        offs[j + 1] = at
    return b"".join(strings), offs


def SortPickSplitters(keys, max_bins=SORT_BINS):
    """bsk_sort_pick_splitters (no device): at most max_bins - 1 strictly ascending splitters at the quantiles of `keys`"""
    blob, offs = _pack_strings(keys)
    out = C.create_string_buffer(max(1, len(blob)))
    o = (C.c_uint64 * max_bins)()
    k = C.c_uint32()
    check(lib.bsk_sort_pick_splitters(blob, offs, len(keys), max_bins, out, len(blob), o, C.byref(k)))
    return [out.raw[o[j]:o[j + 1]] for j in range(k.value)]


def SortSampleRun(op, input, rate):
    """bsk_sort_sample_run over the shards of `input`, in order: the record count of every shard (the sample accumulates in
    the operator's context)"""
    return _count_pass(lib.bsk_sort_sample_run, op, input, rate)


def SortSampleReset(op):
    check(lib.bsk_sort_sample_reset(op.ctx), op.ctx)


def SortSampleCount(op):
    k = C.c_uint64()
    check(lib.bsk_sort_sample_count(op.ctx, C.byref(k)), op.ctx)
    return k.value


def SortSplittersBuild(op, max_bins=SORT_BINS):
    """bsk_sort_splitters_build: splitters from the context's sample, installed; the number of fine bins"""
    k = C.c_uint32()
    check(lib.bsk_sort_splitters_build(op.ctx, max_bins, C.byref(k)), op.ctx)
    return k.value


def SortSplittersSet(op, splitters):
    """bsk_sort_splitters_set: splitters (byte strings, strictly ascending under the padded comparison) installed by hand"""
    blob, offs = _pack_strings(splitters)
    check(lib.bsk_sort_splitters_set(op.ctx, blob, offs, len(splitters)), op.ctx)


def SortSplittersGet(op):
    """bsk_sort_splitters_get: the installed splitters"""
    k, nb = C.c_uint32(), C.c_uint64()
    check(lib.bsk_sort_splitters_get(op.ctx, None, 0, None, C.byref(k), C.byref(nb)), op.ctx)
    buf = C.create_string_buffer(max(1, nb.value))
    offs = (C.c_uint64 * (k.value + 1))()
    check(lib.bsk_sort_splitters_get(op.ctx, buf, nb.value, offs, C.byref(k), C.byref(nb)), op.ctx)
    return [buf.raw[offs[j]:offs[j + 1]] for j in range(k.value)]


def SortHistRun(op, input):
    """bsk_sort_hist_run over the shards of `input`, in order: the record count of every shard"""
    return _count_pass(lib.bsk_sort_hist_run, op, input)


def SortHistGet(op):
    """bsk_sort_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("sort", op)


def SortHistReset(op):
    _hist_reset("sort", op)


def SortBucket(op, input, counts, lo_bin, hi_bin):
    """bsk_sort_bucket_begin / _add over the shards of `input`, in order / _finish: the sorted bytes of the bucket [lo_bin, hi_bin)"""
    return _out_bucket("sort", op, input, counts, lo_bin, hi_bin)


def SortBucketsPlan(op, input, o, budget_bytes, splitters=None, rate=None, device=0):
    """The passes of SortBuckets in front of the buckets, on an open Sort operator: the splitters (given by hand, or built from
    a sample of the keys at `rate`; default: about SORT_SAMPLES_PER_BIN samples per fine bin, from a count of the records --
    Count(input), one more index pass over every shard; a caller that knows the number of records passes the rate),
    the histogram and the plan (ShufflePlan).  Returns the buckets [(lo_bin, hi_bin)] in output order -- from the last to
    the first with Reverse -- and the record count of every shard."""
    if splitters is None:
        if rate is None:
            total = sum(Count(input, device))
            rate = min(1.0, SORT_SAMPLES_PER_BIN * SORT_BINS / max(1, total))
        SortSampleReset(op)
        SortSampleRun(op, input, rate)
        SortSplittersBuild(op)
    else:
        SortSplittersSet(op, splitters)
    SortHistReset(op)
    counts = SortHistRun(op, input)
    bounds = ShufflePlan(SortHistGet(op)[0], budget_bytes)
    buckets = list(zip(bounds[:-1], bounds[1:]))
    if json.loads(o.to_json()).get("Reverse"):
        buckets.reverse()
    return buckets, counts


def SortBuckets(input, o=None, budget_bytes=1 << 30, device=0, splitters=None, rate=None):
    """Sort of an input of any size on one device (PARITY SORT, "Buckets"): a sample of the keys gives the splitters, the
    histogram over all shards the plan of buckets of at most `budget_bytes`, then one collect sequence per bucket, every
    bucket sorted by Sort's own code; the same bytes as Sort.  The input is read twice plus once per bucket -- and once more,
    by the index pass alone, for the count of the records that gives the default sample rate (`rate` given: not)."""
    o = o or SeqKitSortOptions()
    with Operator("Sort", o.to_json(), device) as op:
        buckets, counts = SortBucketsPlan(op, input, o, budget_bytes, splitters, rate, device)
        return b"".join(SortBucket(op, input, counts, lo, hi) for lo, hi in buckets)


RMDUP_BINS = _BUCKET_BINS
RMDUP_BUCKET_RECORD_BYTES = 32   # BSK_RMDUP_BUCKET_RECORD_BYTES of include/bsk.h


def RmDupHistRun(op, input):
    """bsk_rmdup_hist_run over the shards of `input`, in order: the record count of every shard (the histogram accumulates
    in the operator's context)"""
    return _count_pass(lib.bsk_rmdup_hist_run, op, input)


def RmDupHistGet(op):
    """bsk_rmdup_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("rmdup", op)


def RmDupHistReset(op):
    _hist_reset("rmdup", op)


def RmDupVerdictBegin(op, total_records):
    """bsk_rmdup_verdict_begin: a zeroed removed-bitmap for the records [0, total_records), no bin decided"""
    check(lib.bsk_rmdup_verdict_begin(op.ctx, total_records), op.ctx)


def RmDupVerdictGet(op, first, count):
    """bsk_rmdup_verdict_get: one byte per record of [first, first + count), 1 = removed"""
    buf = (C.c_uint8 * max(1, count))()
    check(lib.bsk_rmdup_verdict_get(op.ctx, first, count, buf), op.ctx)
    return bytes(buf[:count])


def RmDupBucket(op, input, counts, lo_bin, hi_bin):
    """bsk_rmdup_bucket_begin / _add over the shards of `input`, in order / _finish: (removed, flagged) of the bucket [lo_bin, hi_bin)"""
    return _counted_bucket("rmdup", op, input, counts, lo_bin, hi_bin)


def RmDupEmit(op, input, counts):
    """bsk_rmdup_emit_run over the shards of `input`, in order: the survivors, joined"""
    return _emit_pass(lib.bsk_rmdup_emit_run, op, input, counts)


def RmDupBuckets(input, o=None, budget_bytes=1 << 30, device=0):
    """RmDup of an input of any size on one device (PARITY RMDUPB): the histogram of the fine bins of the key over all shards,
    the plan of buckets of at most `budget_bytes` of subjects, one collect sequence per bucket, which ends in the bucket's
    share of the verdict, and one emit pass; the same bytes as RmDup.  The input is read twice plus once per bucket."""
    with Operator("RmDup", (o or SeqKitRmDupOptions()).to_json(), device) as op:
        RmDupHistReset(op)
        counts = RmDupHistRun(op, input)
        bounds = ShufflePlan(RmDupHistGet(op)[0], budget_bytes)
        RmDupVerdictBegin(op, sum(counts))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            RmDupBucket(op, input, counts, lo, hi)
        return RmDupEmit(op, input, counts)


def RenameHistRun(op, input):
    """bsk_rename_hist_run over the shards of `input`, in order: the record count of every shard (the histogram accumulates
    in the operator's context)"""
    return _count_pass(lib.bsk_rename_hist_run, op, input)


def RenameHistGet(op):
    """bsk_rename_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("rename", op)


def RenameHistReset(op):
    _hist_reset("rename", op)


def RenameVerdictBegin(op, total_records):
    """bsk_rename_verdict_begin: zeroed ordinals for the records [0, total_records), no bin decided"""
    check(lib.bsk_rename_verdict_begin(op.ctx, total_records), op.ctx)


def RenameVerdictGet(op, first, count):
    """bsk_rename_verdict_get: the ordinal of every record of [first, first + count) inside its group of equal subjects"""
    buf = (C.c_uint32 * max(1, count))()
    check(lib.bsk_rename_verdict_get(op.ctx, first, count, buf), op.ctx)
    return list(buf[:count])


def RenameBucket(op, input, counts, lo_bin, hi_bin):
    """bsk_rename_bucket_begin / _add over the shards of `input`, in order / _finish: (renamed, flagged) of the bucket [lo_bin, hi_bin)"""
    return _counted_bucket("rename", op, input, counts, lo_bin, hi_bin)


def RenameEmit(op, input, counts):
    """bsk_rename_emit_run over the shards of `input`, in order: the records, renamed, joined"""
    return _emit_pass(lib.bsk_rename_emit_run, op, input, counts)


def RenameBuckets(input, o=None, budget_bytes=1 << 30, device=0):
    """Rename of an input of any size on one device (PARITY RENB): the histogram of the fine bins of the key over all shards, the
    plan of buckets of at most `budget_bytes` of subjects, one collect sequence per bucket, which ends in the bucket's share of
    the ordinals, and one emit pass; the same bytes as Rename.  The input is read twice plus once per bucket; the ordinals
    (4 bytes per record of the input) lie outside the budget."""
    with Operator("Rename", (o or SeqKitRenameOptions()).to_json(), device) as op:
        RenameHistReset(op)
        counts = RenameHistRun(op, input)
        bounds = ShufflePlan(RenameHistGet(op)[0], budget_bytes)
        RenameVerdictBegin(op, sum(counts))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            RenameBucket(op, input, counts, lo, hi)
        return RenameEmit(op, input, counts)


def _union_frame(inputs):
    """the shards of the files of `common`, in command order, as one frame: the global record index runs over all of them"""
    if any(f.format != inputs[0].format for f in inputs):
        raise ValueError("common: inputs of different formats")
    return SeqFrame(inputs[0].format, [s for f in inputs for s in f.shards])


def CommonHistRun(op, inputs):
    """bsk_common_hist_run over the shards of every file of `inputs`, in order: per file, the record count of every shard (the
    histogram accumulates in the operator's context)"""
    flat = _count_pass(lib.bsk_common_hist_run, op, _union_frame(inputs))
    counts, at = [], 0
    for f in inputs:
        counts.append(flat[at:at + len(f.shards)])
        at += len(f.shards)
    return counts


def CommonHistGet(op):
    """bsk_common_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("common", op)


def CommonHistReset(op):
    _hist_reset("common", op)


def CommonVerdictBegin(op, file_records):
    """bsk_common_verdict_begin: zeroed keep bits for the records of the first file, no bin decided; file_records[f] = the
    records of file f (2 .. 64 files)"""
    arr = (C.c_uint64 * max(1, len(file_records)))(*file_records)
    check(lib.bsk_common_verdict_begin(op.ctx, arr, len(file_records)), op.ctx)


def CommonVerdictGet(op, first, count):
    """bsk_common_verdict_get: one byte per record of [first, first + count) of the first file, 1 = kept"""
    buf = (C.c_uint8 * max(1, count))()
    check(lib.bsk_common_verdict_get(op.ctx, first, count, buf), op.ctx)
    return bytes(buf[:count])


def CommonBucket(op, inputs, counts, lo_bin, hi_bin):
    """bsk_common_bucket_begin / _add over the shards of every file of `inputs`, in order, the first file first / _finish:
    (kept, flagged) of the bucket [lo_bin, hi_bin); `counts` is what CommonHistRun returned"""
    return _counted_bucket("common", op, _union_frame(inputs), [k for c in counts for k in c], lo_bin, hi_bin)


def CommonEmit(op, input, counts):
    """bsk_common_emit_run over the shards of the FIRST file, in order (`counts`: the record count of each): the kept records, joined"""
    return _emit_pass(lib.bsk_common_emit_run, op, input, counts)


def CommonBuckets(inputA, inputB, o=None, *inputN, budget_bytes=1 << 30, device=0):
    """Common of files of any size on one device (PARITY COMB): the histogram of the fine bins of the key over the shards of all
    files, the plan of buckets of at most `budget_bytes` of subjects, one collect sequence per bucket over all files, which ends
    in the bucket's share of the keep bits of the first file, and one emit pass over the first file; the same bytes as Common.
    The files are read once plus once per bucket, the first file once more.  An empty file gives an empty result."""
    inputs = [inputA, inputB, *inputN]
    with Operator("Common", (o or SeqKitCommonOptions()).to_json(), device) as op:
        CommonHistReset(op)
        counts = CommonHistRun(op, inputs)
        bounds = ShufflePlan(CommonHistGet(op)[0], budget_bytes)
        CommonVerdictBegin(op, [sum(c) for c in counts])
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            CommonBucket(op, inputs, counts, lo, hi)
        return CommonEmit(op, inputA, counts[0])


def _pair_frames(inputA, inputB):
    if inputA.format != inputB.format:
        raise ValueError("pair: inputs of different formats")
    return [inputA, inputB]


def PairHistRun(op, inputs):
    """bsk_pair_hist_run over the shards of file 1, then file 2: per file, the record count of every shard (the histogram
    accumulates in the operator's context)"""
    flat = _count_pass(lib.bsk_pair_hist_run, op, _union_frame(inputs))
    na = len(inputs[0].shards)
    return [flat[:na], flat[na:]]


def PairHistGet(op):
    """bsk_pair_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("pair", op)


def PairHistReset(op):
    _hist_reset("pair", op)


def PairVerdictBegin(op, file_records):
    """bsk_pair_verdict_begin: zeroed paired bits for the records of both files, no bin decided; file_records = [n1, n2]"""
    arr = (C.c_uint64 * 2)(*file_records)
    check(lib.bsk_pair_verdict_begin(op.ctx, arr), op.ctx)


def PairVerdictGet(op, first, count):
    """bsk_pair_verdict_get: pos of the global records [first, first + count) after PairOrderBegin; None = unpaired"""
    buf = (C.c_uint64 * max(1, count))()
    check(lib.bsk_pair_verdict_get(op.ctx, first, count, buf), op.ctx)
    return [None if v == 0xFFFFFFFFFFFFFFFF else v for v in buf[:count]]


def PairBucket(op, inputs, counts, lo_bin, hi_bin):
    """bsk_pair_bucket_begin / _add over the shards of file 1, then file 2 / _finish: (pairs, flagged) of the match bucket
    [lo_bin, hi_bin); `counts` is what PairHistRun returned"""
    return _counted_bucket("pair", op, _union_frame(inputs), [k for c in counts for k in c], lo_bin, hi_bin)


def PairOrderBegin(op):
    """bsk_pair_order_begin, the rank step: (P, file 2 is in mate order)"""
    pairs, ordered = C.c_uint64(), C.c_int()
    check(lib.bsk_pair_order_begin(op.ctx, None, C.byref(pairs), C.byref(ordered)), op.ctx)
    return pairs.value, bool(ordered.value)


def PairEmit(op, input, counts, first):
    """bsk_pair_emit_run over the shards of ONE file, in order, the first of them global record `first` (`counts`: the record
    count of each): the three outputs of the entry point, each joined over the shards"""
    chunks = ([], [], [])
    for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), counts):
        outs = (_lib.Out * 3)()
        check(lib.bsk_pair_emit_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None, outs), op.ctx)
        for k in range(3):
            chunks[k].append(_out_bytes(op, outs[k]))
        first += cnt
    return tuple(b"".join(c) for c in chunks)


def PairOrderHistRun(op, input, counts, first):
    """bsk_pair_order_hist_run over the shards of file 2, in order, the first of them global record `first`"""
    _count_pass(lib.bsk_pair_order_hist_run, op, input, counts=counts, first=first)


def PairOrderHistGet(op):
    """bsk_pair_order_hist_get: (bytes[4096], records[4096]) of the order bins"""
    return _hist_get("pair_order", op)


def PairOrderBucket(op, input, counts, first, lo_bin, hi_bin):
    """bsk_pair_order_bucket_begin / _add over the shards of file 2 / _finish: the share of paired.2 of the order bucket
    [lo_bin, hi_bin)"""
    return _out_bucket("pair_order", op, input, counts, lo_bin, hi_bin, first)


def PairBuckets(inputA, inputB, o=None, budget_bytes=1 << 30, device=0, order="auto"):
    """Pair of two files of any size on one device (PARITY PAIRB) -> (paired.1, paired.2, unpaired.1, unpaired.2), the same
    bytes as Pair.  The match phase: the histogram of the fine bins of the key over both files, the plan of buckets of at most
    `budget_bytes` of subjects, one collect sequence per bucket, which ends in the bucket's share of the paired bits and the
    mates.  Then the rank step and one emit pass over either file.  When file 2 is not in the order of its mates -- or with
    order="buckets" -- paired.2 comes from the order phase: the histogram of the positions over file 2, the plan under the
    same budget, one collect sequence per bucket."""
    if order not in ("auto", "buckets"):
        raise ValueError("PairBuckets: order is 'auto' or 'buckets'")
    inputs = _pair_frames(inputA, inputB)
    with Operator("Pair", (o or SeqKitPairOptions()).to_json(), device) as op:
        if order == "buckets":
            check(lib.bsk_ctx_set(op.ctx, b"pair_order", b"buckets"), op.ctx)
        PairHistReset(op)
        counts = PairHistRun(op, inputs)
        bounds = ShufflePlan(PairHistGet(op)[0], budget_bytes)
        n1 = sum(counts[0])
        PairVerdictBegin(op, [n1, sum(counts[1])])
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            PairBucket(op, inputs, counts, lo, hi)
        pairs, ordered = PairOrderBegin(op)
        paired1, unpaired1, _ = PairEmit(op, inputA, counts[0], 0)
        _, unpaired2, paired2 = PairEmit(op, inputB, counts[1], n1)
        if pairs and (order == "buckets" or not ordered):
            PairOrderHistRun(op, inputB, counts[1], n1)
            obounds = ShufflePlan(PairOrderHistGet(op)[0], budget_bytes)
            paired2 = b"".join(PairOrderBucket(op, inputB, counts[1], n1, lo, hi) for lo, hi in zip(obounds[:-1], obounds[1:]))
        return paired1, paired2, unpaired1, unpaired2


def _concat_frames(inputA, inputB):
    if inputA.format != inputB.format:
        raise ValueError("concat: inputs of different formats")
    return [inputA, inputB]


def ConcatHistRun(op, inputs):
    """bsk_concat_hist_run over the shards of file 1, then file 2: per file, the record count of every shard (the histogram
    accumulates in the operator's context)"""
    flat = _count_pass(lib.bsk_concat_hist_run, op, _union_frame(inputs))
    na = len(inputs[0].shards)
    return [flat[:na], flat[na:]]


def ConcatHistGet(op):
    """bsk_concat_hist_get: (bytes[4096], records[4096])"""
    return _hist_get("concat", op)


def ConcatHistReset(op):
    _hist_reset("concat", op)


def ConcatVerdictBegin(op, file_records):
    """bsk_concat_verdict_begin: a head word for the records of both files, no bin decided; file_records = [n1, n2]"""
    arr = (C.c_uint64 * 2)(*file_records)
    check(lib.bsk_concat_verdict_begin(op.ctx, arr), op.ctx)


def ConcatVerdictGet(op, first, count):
    """bsk_concat_verdict_get: head of the global records [first, first + count); None = file 1 has no record of that ID"""
    buf = (C.c_uint64 * max(1, count))()
    check(lib.bsk_concat_verdict_get(op.ctx, first, count, buf), op.ctx)
    return [None if v == 0xFFFFFFFFFFFFFFFF else v for v in buf[:count]]


def ConcatBucket(op, inputs, counts, lo_bin, hi_bin):
    """bsk_concat_bucket_begin / _add over the shards of file 1, then file 2 / _finish: (matched, flagged) of the match bucket
    [lo_bin, hi_bin); `counts` is what ConcatHistRun returned"""
    return _counted_bucket("concat", op, _union_frame(inputs), [k for c in counts for k in c], lo_bin, hi_bin)


def ConcatJoinBegin(op):
    """bsk_concat_join_begin: zeroed weights, mark bits and window histogram, once every bin is decided"""
    check(lib.bsk_concat_join_begin(op.ctx, None), op.ctx)


def ConcatWeighRun(op, input, counts, first):
    """bsk_concat_weigh_run over the shards of file 2, in order, the first of them global record `first`"""
    _count_pass(lib.bsk_concat_weigh_run, op, input, counts=counts, first=first)


def ConcatWindowHistRun(op, input, counts):
    """bsk_concat_window_hist_run over the shards of file 1, in order"""
    _count_pass(lib.bsk_concat_window_hist_run, op, input, counts=counts)


def ConcatWindowHistGet(op):
    """bsk_concat_window_hist_get: (cost[4096], records[4096]) of the window bins"""
    return _hist_get("concat_window", op)


def ConcatWindowShift(n1):
    """the least shift s with (n1 - 1) >> s < 4096 (0 for an empty file 1)"""
    s = 0
    while n1 and (n1 - 1) >> s >= _BUCKET_BINS:
        s += 1
    return s


def ConcatWindow(op, inputs, counts, lo_bin, hi_bin):
    """bsk_concat_window_begin / _add over the shards of file 1 that reach into the window, then every shard of file 2 /
    _finish: the share of the output of the window [lo_bin, hi_bin)"""
    n1 = sum(counts[0])
    s = ConcatWindowShift(n1)
    check(lib.bsk_concat_window_begin(op.ctx, lo_bin, hi_bin), op.ctx)
    first = 0
    for f, (input, cnts) in enumerate(zip(inputs, counts)):
        for (pid, ptr, n, on_dev, keep), cnt in zip(input.partitions(), cnts):
            outside = f == 0 and (cnt == 0 or (first + cnt - 1) >> s < lo_bin or first >> s >= hi_bin)
            if not outside:
                check(lib.bsk_concat_window_add(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, first, None), op.ctx)
            first += cnt
    out = _lib.Out()
    check(lib.bsk_concat_window_finish(op.ctx, None, C.byref(out)), op.ctx)
    return _out_bytes(op, out)


def ConcatTail(op, input, counts, first):
    """bsk_concat_tail_run over the shards of file 2, in order, the first of them global record `first`: with Full the records
    of file 2 whose ID file 1 does not have, joined; else empty"""
    return _emit_pass(lib.bsk_concat_tail_run, op, input, counts, first)


def ConcatBuckets(inputA, inputB, o=None, budget_bytes=1 << 30, device=0):
    """Concat of two files of any size on one device (PARITY CONB) -> the same bytes as Concat.  The match phase: the histogram
    of the fine bins of the key over both files, the plan of buckets of at most `budget_bytes` of subjects, one collect sequence
    per bucket, which ends in the bucket's share of the heads.  The join phase: the weights of the heads over file 2, the
    histogram of the window costs over file 1, the plan of windows under the same budget -- a window bin above it is refused by
    the plan, which names its bytes --, one collect sequence per window, and with Full the tail over file 2."""
    inputs = _concat_frames(inputA, inputB)
    with Operator("Concat", (o or SeqKitConcatOptions()).to_json(), device) as op:
        ConcatHistReset(op)
        counts = ConcatHistRun(op, inputs)
        bounds = ShufflePlan(ConcatHistGet(op)[0], budget_bytes)
        n1 = sum(counts[0])
        ConcatVerdictBegin(op, [n1, sum(counts[1])])
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            ConcatBucket(op, inputs, counts, lo, hi)
        ConcatJoinBegin(op)
        ConcatWeighRun(op, inputB, counts[1], n1)
        ConcatWindowHistRun(op, inputA, counts[0])
        wbounds = ShufflePlan(ConcatWindowHistGet(op)[0], budget_bytes)
        chunks = [ConcatWindow(op, inputs, counts, lo, hi) for lo, hi in zip(wbounds[:-1], wbounds[1:])]
        chunks.append(ConcatTail(op, inputB, counts[1], n1))
        return b"".join(chunks)


def HeadGenome(input, o=None, device=0):
    """bigseqkit/head_genome.go:37-77 (PARITY HEADG): the records of the first genome.  ONE cut over the whole input: the
    shards go through one context in order, which carries the prefix words, n_1 and "cut reached" from shard to shard, and
    nothing is launched for the shards behind the cut."""
    chunks = []
    with Operator("HeadGenome", (o or SeqKitHeadGenomeOptions()).to_json(), device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            out = _lib.Out()
            check(lib.bsk_head_genome_run(op.ctx, ptr, n, 1 if on_dev else 0, input.format, pid, None, C.byref(out)), op.ctx)
            chunks.append(_out_bytes(op, out))
            cut = C.c_int()
            check(lib.bsk_head_genome_state(op.ctx, C.byref(cut), None), op.ctx)
            if cut.value:
                break
    return b"".join(chunks)


def build_index(input, device=0):
    """Record table of the first shard (tests): list of (start, head_len, seq_len, aux)."""
    with Operator("SeqTransform", "{}", device) as op:
        for pid, ptr, n, on_dev, keep in input.partitions():
            nrec = C.c_uint64()
            check(lib.bsk_index_build(op.ctx, ptr, n, 1 if on_dev else 0, input.format, None, C.byref(nrec)), op.ctx)
            k = nrec.value
            st, hl, sl, ax = (C.c_uint64 * k)(), (C.c_uint32 * k)(), (C.c_uint32 * k)(), (C.c_uint32 * k)()
            check(lib.bsk_index_copy(op.ctx, st, hl, sl, ax, k), op.ctx)
            return list(zip(st, hl, sl, ax))
    return []
