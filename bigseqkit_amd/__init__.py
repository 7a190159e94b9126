"""bigseqkit_amd -- MI355X-native engine behind BigSeqKit's per-record hot path.

The product is libbsk.so (hand-written HIP for gfx950 behind the C ABI in
include/bsk.h).  This package is the thin host-side mirror of the reference's
driver library used by tests and bench.py; it has no CPU fallback.
"""
from ._lib import BskError, FORMAT_FASTA, FORMAT_FASTQ, lib  # noqa: F401  (fails loudly if libbsk.so is missing)
from .options import (SeqKitConfig, SeqKitStatsOptions, SeqKitSeqOptions, SeqKitGrepOptions,  # noqa: F401
                      SeqKitLocateOptions, SeqKitSubseqOptions, SeqKitTranslateOptions, SeqKitRmDupOptions,
                      SeqKitFq2FaOptions, SeqKitRangeOptions, SeqKitHeadOptions, SeqKitDuplicateOptions, SeqKitRenameOptions, SeqKitSortOptions, SeqKitFaidxOptions, SeqKitPairOptions, SeqKitCommonOptions, SeqKitConcatOptions, SeqKitReplaceOptions, SeqKitFa2FqOptions, SeqKitSampleOptions,
                      SeqKitShuffleOptions, SeqKitHeadGenomeOptions)
from .api import (SeqFrame, BgzfProbe, BgzfInflate, GzipInflate, GzipPlan, BgzfBlocks, BgzfReader, BgzfCutPoints, BgzfShardLoad,GzipReader, BgzfDeflate, BgzfDeflateHost, ReadSeqFile, WriteSeqFile, ReadFASTA, ReadFASTAN, ReadFASTQ, ReadFASTQN, Operator, Stats, StatsString,  # noqa: F401
                  stats_map, Seq, build_index, Grep, GrepCount, Subseq, Translate, RmDup, Locate, Fq2Fa, Range, Head,
                  Duplicate, Count, Rename, Sort, Faidx, Pair, Common, Concat, FaidxQuery, FaidxFetch, FaidxFetchPlan, BgzfGzi, Replace, Fa2Fq, Sample, Shuffle, ShuffleBuckets, ShuffleHistRun, ShuffleHistGet, ShuffleHistReset, ShufflePlan, ShuffleBucket, HeadGenome,
                  SortBuckets, SortBucketsPlan, SortBucket, SortSampleRun, SortSampleReset, SortSampleCount, SortPickSplitters, SortSplittersBuild,
                  SortSplittersSet, SortSplittersGet, SortHistRun, SortHistGet, SortHistReset,
                  RmDupBuckets, RmDupHistRun, RmDupHistGet, RmDupHistReset, RmDupVerdictBegin, RmDupVerdictGet, RmDupBucket, RmDupEmit,
                  RenameBuckets, RenameHistRun, RenameHistGet, RenameHistReset, RenameVerdictBegin, RenameVerdictGet, RenameBucket, RenameEmit,
                  CommonBuckets, CommonHistRun, CommonHistGet, CommonHistReset, CommonVerdictBegin, CommonVerdictGet, CommonBucket, CommonEmit,
                  PairBuckets, PairHistRun, PairHistGet, PairHistReset, PairVerdictBegin, PairVerdictGet, PairBucket, PairOrderBegin, PairEmit,
                  PairOrderHistRun, PairOrderHistGet, PairOrderBucket,
                  ConcatBuckets, ConcatHistRun, ConcatHistGet, ConcatHistReset, ConcatVerdictBegin, ConcatVerdictGet, ConcatBucket,
                  ConcatJoinBegin, ConcatWeighRun, ConcatWindowHistRun, ConcatWindowHistGet, ConcatWindowShift, ConcatWindow, ConcatTail)
