"""abpoa_amd — MI355X-native partial order alignment (abPOA-compatible).

Thin ctypes access to the native library for tests and bench. The compute
path is the HIP/CDNA4 core inside libabpoa_amd.so; this package performs no
alignment math in Python.
"""
import ctypes
import os

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libabpoa_amd.so")
CLI_PATH = os.path.join(_CSRC, "abpoa_amd")
CLI_CPUTEST_PATH = os.path.join(_CSRC, "abpoa_amd_cputest")
ORACLE_SO = os.path.join(os.path.dirname(_CSRC), os.pardir, "oracle", "liboracle.so")

_lib = None


def lib():
    """Load (once) and return the native library handle."""
    global _lib
    if _lib is None:
        path = os.environ.get("ABPOA_AMD_LIB", LIB_PATH)
        if not os.path.exists(path):
            raise RuntimeError("libabpoa_amd.so not built; run __graft_entry__.build()")
        _lib = ctypes.CDLL(path)
        _lib.abpoa_amd_get_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 3
        _lib.abpoa_amd_get_stats.restype = None
        _lib.abpoa_amd_reset_stats.restype = None
    return _lib


def get_stats():
    """(dp_cells, kernel_ns, n_launches) accumulated by the native core."""
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib().abpoa_amd_get_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def reset_stats():
    lib().abpoa_amd_reset_stats()


class ConsT(ctypes.Structure):
    """Mirror of abpoa_cons_t (include/abpoa_amd.h)."""
    _fields_ = [
        ("n_cons", ctypes.c_int), ("n_seq", ctypes.c_int), ("msa_len", ctypes.c_int),
        ("clu_n_seq", ctypes.POINTER(ctypes.c_int)),
        ("clu_read_ids", ctypes.POINTER(ctypes.POINTER(ctypes.c_int))),
        ("cons_len", ctypes.POINTER(ctypes.c_int)),
        ("cons_node_ids", ctypes.POINTER(ctypes.POINTER(ctypes.c_int))),
        ("cons_base", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
        ("msa_base", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
        ("cons_cov", ctypes.POINTER(ctypes.POINTER(ctypes.c_int))),
        ("cons_phred_score", ctypes.POINTER(ctypes.POINTER(ctypes.c_int))),
    ]


CONS_CB = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.POINTER(ConsT), ctypes.c_void_p)


def get_cons_stats():
    """Consensus-stage counters of the batched driver since the last reset:
    dict(device_sets, host_sets, fallback_sets, d2h_bytes, kernel_ns).
    device_sets took the GPU consensus kernel; host_sets downloaded their graph
    for the host pass (fallback_sets of them after a non-OK device status)."""
    L = lib()
    L.abpoa_amd_get_cons_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 5
    L.abpoa_amd_get_cons_stats.restype = None
    v = [ctypes.c_uint64() for _ in range(5)]
    L.abpoa_amd_get_cons_stats(*[ctypes.byref(x) for x in v])
    keys = ("device_sets", "host_sets", "fallback_sets", "d2h_bytes", "kernel_ns")
    return dict(zip(keys, (x.value for x in v)))


def reset_cons_stats():
    L = lib()
    L.abpoa_amd_reset_cons_stats.restype = None
    L.abpoa_amd_reset_cons_stats()


def get_msa_stats():
    """Row-column MSA counters of the batched driver since the last reset, for
    calls with out_msa only: dict(device_sets, host_sets, fallback_sets,
    d2h_bytes, kernel_ns). device_sets had their rows built by the GPU MSA
    kernels; host_sets downloaded their graph for abpoa_generate_rc_msa
    (fallback_sets of them after a non-OK device status)."""
    L = lib()
    L.abpoa_amd_get_msa_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 5
    L.abpoa_amd_get_msa_stats.restype = None
    v = [ctypes.c_uint64() for _ in range(5)]
    L.abpoa_amd_get_msa_stats(*[ctypes.byref(x) for x in v])
    keys = ("device_sets", "host_sets", "fallback_sets", "d2h_bytes", "kernel_ns")
    return dict(zip(keys, (x.value for x in v)))


def reset_msa_stats():
    L = lib()
    L.abpoa_amd_reset_msa_stats.restype = None
    L.abpoa_amd_reset_msa_stats()


_MULTICONS_KEYS = ("device_sets", "host_sets", "fallback_sets", "one_cluster_sets",
                   "clusters", "cand_cols", "d2h_bytes", "kernel_ns")


def get_multicons_stats():
    """Multi-consensus counters of the batched driver since the last reset, for
    calls with max_n_cons > 1 made under ABPOA_AMD_DEVICE_MULTICONS only:
    dict(device_sets, host_sets, fallback_sets, one_cluster_sets, clusters,
    cand_cols, d2h_bytes, kernel_ns). device_sets had their candidate columns
    found, and their per-cluster consensus computed, on the GPU; host_sets
    downloaded their graph (fallback_sets of them after a non-OK device
    status); one_cluster_sets / clusters / cand_cols describe the device sets."""
    L = lib()
    L.abpoa_amd_get_multicons_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * len(_MULTICONS_KEYS)
    L.abpoa_amd_get_multicons_stats.restype = None
    v = [ctypes.c_uint64() for _ in _MULTICONS_KEYS]
    L.abpoa_amd_get_multicons_stats(*[ctypes.byref(x) for x in v])
    return dict(zip(_MULTICONS_KEYS, (x.value for x in v)))


def reset_multicons_stats():
    L = lib()
    L.abpoa_amd_reset_multicons_stats.restype = None
    L.abpoa_amd_reset_multicons_stats()


def get_fold_stats():
    """Graph-fold counters of the batched driver since the last reset:
    dict(parallel_folds, fallback_folds, serial_folds). parallel_folds ran the
    lane-parallel mutation walk; fallback_folds tripped one of its checks and
    were redone by the serial walk; serial_folds ran the serial walk because
    ABPOA_AMD_SERIAL_FOLD was set."""
    L = lib()
    L.abpoa_amd_get_fold_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 3
    L.abpoa_amd_get_fold_stats.restype = None
    v = [ctypes.c_uint64() for _ in range(3)]
    L.abpoa_amd_get_fold_stats(*[ctypes.byref(x) for x in v])
    keys = ("parallel_folds", "fallback_folds", "serial_folds")
    return dict(zip(keys, (x.value for x in v)))


def reset_fold_stats():
    L = lib()
    L.abpoa_amd_reset_fold_stats.restype = None
    L.abpoa_amd_reset_fold_stats()


_BATCH_KEYS = ("resident_calls", "hostfold_calls", "dp_retry_jobs", "dp_retry_launches",
               "pool_expands", "big_chunks", "noop_folds", "seam_retry_jobs",
               "launches_i16", "launches_i32")


def get_batch_stats():
    """Path counters of the batched drivers since the last reset, as a dict:
    resident_calls / hostfold_calls (which driver served each msa_batch call),
    dp_retry_jobs / dp_retry_launches (DP arena overflows of the resident
    driver and the launches that redid them), pool_expands, big_chunks,
    noop_folds (empty CIGAR on an existing graph), seam_retry_jobs (arena
    overflows of the aligner seam), launches_i16 / launches_i32 (resident DP
    launches by score width)."""
    L = lib()
    L.abpoa_amd_get_batch_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * len(_BATCH_KEYS)
    L.abpoa_amd_get_batch_stats.restype = None
    v = [ctypes.c_uint64() for _ in _BATCH_KEYS]
    L.abpoa_amd_get_batch_stats(*[ctypes.byref(x) for x in v])
    return dict(zip(_BATCH_KEYS, (x.value for x in v)))


def reset_batch_stats():
    L = lib()
    L.abpoa_amd_reset_batch_stats.restype = None
    L.abpoa_amd_reset_batch_stats()


_ACGT = "ACGTN-"
_ROW_TR = bytes(_ACGT.encode("ascii") + b"?" * (256 - len(_ACGT)))


def msa_batch_results(sets, n_threads=4, cons_algrm=None, max_n_cons=1,
                      out_msa=False, out_cons=True, scoring=None):
    """Run the batched GPU driver over `sets` (list of list of bytes, codes
    0..3) and return, per set, the full callback payload as a dict:
      cons          list of consensus strings (one per cluster)
      node_ids/cov/phred   per-cluster lists of ints, one entry per base
      clu_n_seq     reads per cluster
      clu_read_ids  per-cluster read-id lists
      n_seq         reads in the set
    cons_algrm: None = library default (HB), "MF" = most-frequent (exercises
    the per-edge read-id bitsets on the device-resident path).
    max_n_cons: 1, 2 or 3 consensus sequences per set.
    out_msa: also build the row-column MSA; each result then additionally holds
      msa_len       number of columns
      msa           list of row strings over "ACGTN-": the read rows, then
                    (with out_cons) the consensus rows
    out_cons: with out_msa, whether the consensus rows are part of the MSA
    (the consensus itself is always delivered). Results without out_msa keep
    exactly the keys listed first.
    scoring: optional dict of integer scoring parameters to override, keys
    among match, mismatch, gap_open1, gap_open2, gap_ext1, gap_ext2."""
    L = lib()
    L.abpoa_init_para.restype = ctypes.c_void_p
    L.abpoa_post_set_para.argtypes = [ctypes.c_void_p]
    L.abpoa_free_para.argtypes = [ctypes.c_void_p]
    L.abpoa_amd_msa_batch.argtypes = [
        ctypes.c_void_p, ctypes.c_int,
        ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.POINTER(ctypes.c_int)),
        ctypes.POINTER(ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
        CONS_CB, ctypes.c_void_p, ctypes.c_int]
    para = L.abpoa_init_para()
    if cons_algrm is not None or max_n_cons != 1 or out_msa or scoring:
        from .pyabpoa import ParaT, ABPOA_HB, ABPOA_MF
        p = ctypes.cast(para, ctypes.POINTER(ParaT)).contents
        for key, value in (scoring or {}).items():
            if key not in ("match", "mismatch", "gap_open1", "gap_open2", "gap_ext1", "gap_ext2"):
                raise ValueError("unknown scoring parameter %r" % key)
            setattr(p, key, int(value))
        if cons_algrm is not None:
            p.cons_algrm = {"HB": ABPOA_HB, "MF": ABPOA_MF}[cons_algrm.upper()]
        if max_n_cons != 1:
            if max_n_cons < 1 or max_n_cons > 3:
                raise ValueError("max_n_cons must be 1, 2 or 3")
            p.max_n_cons = max_n_cons
        if out_msa:
            # before abpoa_post_set_para, which switches read-id tracking on
            p.out_msa = 1
            p.out_cons = 1 if out_cons else 0
    L.abpoa_post_set_para(para)

    n_sets = len(sets)
    NSeqs = (ctypes.c_int * n_sets)(*[len(s) for s in sets])
    lens_keep, ptrs_keep, bufs_keep = [], [], []
    for s in sets:
        lens = (ctypes.c_int * len(s))(*[len(r) for r in s])
        lens_keep.append(lens)
        bufs = [ctypes.create_string_buffer(r, len(r)) for r in s]
        bufs_keep.append(bufs)
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * len(s))(
            *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
        ptrs_keep.append(ptrs)
    LensTop = (ctypes.POINTER(ctypes.c_int) * n_sets)(*lens_keep)
    SeqsTop = (ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)) * n_sets)(*ptrs_keep)

    out = [None] * n_sets

    @CONS_CB
    def cb(idx, cons_p, _user):
        c = cons_p.contents
        r = {"n_seq": c.n_seq, "cons": [], "node_ids": [], "cov": [], "phred": [],
             "clu_n_seq": [], "clu_read_ids": []}
        for ci in range(c.n_cons):
            ln = c.cons_len[ci]
            r["cons"].append("".join(_ACGT[b] for b in c.cons_base[ci][:ln]))
            r["node_ids"].append(c.cons_node_ids[ci][:ln])
            r["cov"].append(c.cons_cov[ci][:ln])
            r["phred"].append(c.cons_phred_score[ci][:ln])
            r["clu_n_seq"].append(c.clu_n_seq[ci])
            r["clu_read_ids"].append(c.clu_read_ids[ci][:c.clu_n_seq[ci]])
        if out_msa:
            # rows are valid only during the callback: copy them out here
            ln = c.msa_len
            n_rows = c.n_seq + (c.n_cons if out_cons else 0) if ln > 0 else 0
            r["msa_len"] = ln
            r["msa"] = [ctypes.string_at(c.msa_base[i], ln).translate(_ROW_TR).decode("ascii")
                        for i in range(n_rows)]
        out[idx] = r

    rc = L.abpoa_amd_msa_batch(para, n_sets, NSeqs, LensTop, SeqsTop, cb, None, n_threads)
    L.abpoa_free_para(para)
    assert rc == 0
    return out


def msa_batch_consensus(sets, n_threads=4, cons_algrm=None):
    """Run the batched GPU driver over `sets` (list of list of bytes, codes
    0..3) and return each set's consensus as an ACGT string (a list of
    strings where a set yields several). See msa_batch_results."""
    out = []
    for r in msa_batch_results(sets, n_threads=n_threads, cons_algrm=cons_algrm):
        seqs = r["cons"]
        out.append(seqs[0] if len(seqs) == 1 else seqs)
    return out
