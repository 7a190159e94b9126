"""The key-bucket family keeps its surface: the entry points every prefix shares resolve in libbsk.so under the signatures of
include/bsk.h, written out here and not read from the tables that generate them (bigseqkit_amd/_lib.py), and every public name
of the package is still there.  No device."""
import ctypes as C

import pytest

import bigseqkit_amd
from bigseqkit_amd._lib import lib

_vp, _sz, _i, _i64, _u64, _u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_uint64, C.c_uint32
_p = C.POINTER

HIST_RUN = (_i, [_vp, _vp, _sz, _i, _i, _i64, _u64, _vp, _p(_u64)])
HIST_GET = (_i, [_vp, _p(_u64), _p(_u64)])
HIST_RESET = (_i, [_vp])
BUCKET_BEGIN = (_i, [_vp, _u32, _u32])
BUCKET_ADD = (_i, [_vp, _vp, _sz, _i, _i, _i64, _u64, _vp])

FIVE = {"hist_run": HIST_RUN, "hist_get": HIST_GET, "hist_reset": HIST_RESET, "bucket_begin": BUCKET_BEGIN, "bucket_add": BUCKET_ADD}
FAMILY = {p: dict(FIVE) for p in ("shuffle", "sort", "rmdup", "rename", "common", "pair", "concat")}
# the order buckets of pair: their histogram is reset by bsk_pair_order_begin
FAMILY["pair_order"] = {k: v for k, v in FIVE.items() if k != "hist_reset"}
# the windows of concat, under their own names: reset by bsk_concat_join_begin
FAMILY["concat_window"] = {"hist_run": HIST_RUN, "hist_get": HIST_GET, "begin": BUCKET_BEGIN, "add": BUCKET_ADD}

# the names `from .api import (...)` of bigseqkit_amd/__init__.py listed before the family's glue was folded
PUBLIC_NAMES = """
SeqFrame BgzfProbe BgzfInflate BgzfBlocks ReadSeqFile ReadFASTA ReadFASTAN ReadFASTQ ReadFASTQN Operator Stats StatsString
stats_map Seq build_index Grep GrepCount Subseq Translate RmDup Locate Fq2Fa Range Head
Duplicate Count Rename Sort Faidx Pair Common Concat FaidxQuery Replace Fa2Fq Sample Shuffle ShuffleBuckets ShuffleHistRun
ShuffleHistGet ShuffleHistReset ShufflePlan ShuffleBucket HeadGenome
SortBuckets SortBucketsPlan SortBucket SortSampleRun SortSampleReset SortSampleCount SortPickSplitters SortSplittersBuild
SortSplittersSet SortSplittersGet SortHistRun SortHistGet SortHistReset
RmDupBuckets RmDupHistRun RmDupHistGet RmDupHistReset RmDupVerdictBegin RmDupVerdictGet RmDupBucket RmDupEmit
RenameBuckets RenameHistRun RenameHistGet RenameHistReset RenameVerdictBegin RenameVerdictGet RenameBucket RenameEmit
CommonBuckets CommonHistRun CommonHistGet CommonHistReset CommonVerdictBegin CommonVerdictGet CommonBucket CommonEmit
PairBuckets PairHistRun PairHistGet PairHistReset PairVerdictBegin PairVerdictGet PairBucket PairOrderBegin PairEmit
PairOrderHistRun PairOrderHistGet PairOrderBucket
ConcatBuckets ConcatHistRun ConcatHistGet ConcatHistReset ConcatVerdictBegin ConcatVerdictGet ConcatBucket
ConcatJoinBegin ConcatWeighRun ConcatWindowHistRun ConcatWindowHistGet ConcatWindowShift ConcatWindow ConcatTail
BskError FORMAT_FASTA FORMAT_FASTQ lib
SeqKitConfig SeqKitStatsOptions SeqKitSeqOptions SeqKitGrepOptions SeqKitLocateOptions SeqKitSubseqOptions
SeqKitTranslateOptions SeqKitRmDupOptions SeqKitFq2FaOptions SeqKitRangeOptions SeqKitHeadOptions SeqKitDuplicateOptions
SeqKitRenameOptions SeqKitSortOptions SeqKitFaidxOptions SeqKitPairOptions SeqKitCommonOptions SeqKitConcatOptions
SeqKitReplaceOptions SeqKitFa2FqOptions SeqKitSampleOptions SeqKitShuffleOptions SeqKitHeadGenomeOptions
""".split()


@pytest.mark.parametrize("prefix", sorted(FAMILY))
def test_shared_symbols_resolve_with_their_signatures(prefix):
    for step, (restype, argtypes) in FAMILY[prefix].items():
        fn = getattr(lib, "bsk_%s_%s" % (prefix, step))  # AttributeError: the symbol is gone from the build
        assert fn.restype is restype, (prefix, step, fn.restype)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, (prefix, step, fn.argtypes)


def test_public_names_are_still_there():
    assert len(PUBLIC_NAMES) == len(set(PUBLIC_NAMES))
    missing = [n for n in PUBLIC_NAMES if not hasattr(bigseqkit_amd, n)]
    assert not missing, missing
    family = [n for n in PUBLIC_NAMES if any(n.startswith(p) for p in ("Shuffle", "Sort", "RmDup", "Rename", "Common", "Pair", "Concat"))
              and n not in ("Shuffle", "Sort", "RmDup", "Rename", "Common", "Pair", "Concat")]
    misnamed = [n for n in family if callable(getattr(bigseqkit_amd, n)) and getattr(bigseqkit_amd, n).__name__ != n]
    assert not misnamed, misnamed  # (help() shows every one under its own name)
    # ... and with its docstring: these eight had none before the glue was folded, every other one keeps its own
    bare = {"CommonHistReset", "ConcatHistReset", "PairHistReset", "RenameHistReset", "RmDupHistReset", "SortHistReset", "SortSampleCount",
            "SortSampleReset"}
    undocumented = [n for n in family if callable(getattr(bigseqkit_amd, n)) and n not in bare and not (getattr(bigseqkit_amd, n).__doc__ or "").strip()]
    assert not undocumented, undocumented
