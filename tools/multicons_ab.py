#!/usr/bin/env python3
"""A/B of the multi-consensus stage of the resident batch driver: the default
(graph download, host clustering and consensus) against
ABPOA_AMD_DEVICE_MULTICONS=1 (device rows, het scan, per-cluster consensus).

Generates two-haplotype read sets at the benchmark shape: hap B is hap A with
a SNP every ~500 bases and one short deletion, reads alternate between the
haplotypes and carry bench.gen_sets' errors. In ONE process it runs
max_n_cons = 2 calls with the switch off and on alternately, one warm-up call
each and then --calls timed calls per setting without a callback, and prints
per call the "[abamd timing resident]" phases, the wall, the stage's D2H
bytes, kernel time, candidate columns per set and the device/host/fallback
counts; then one more call per setting with a callback that checksums every
field of every result, which must agree between the settings.

    python tools/multicons_ab.py [--sets 250] [--depth 50] [--qlen 10000]
                                 [--calls 3] [--out-msa] [--max-n-cons 2]
"""
import argparse
import ctypes
import os
import re
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abpoa_amd  # noqa: E402
from abpoa_amd.pyabpoa import ParaT  # noqa: E402

SWITCH = "ABPOA_AMD_DEVICE_MULTICONS"
P_SUB, P_DEL, P_INS = 0.045, 0.03, 0.025   # bench.gen_sets' defaults


def noisy(rng, ref):
    """bench.gen_sets' per-read error model on one template."""
    n = len(ref)
    r = rng.random(n)
    sub = r < P_SUB
    mask_del = (r >= P_SUB) & (r < P_SUB + P_DEL)
    ins = (r >= P_SUB + P_DEL) & (r < P_SUB + P_DEL + P_INS)
    out = ref.copy()
    nsub = int(sub.sum())
    if nsub:
        out[sub] = (ref[sub] + rng.integers(1, 4, size=nsub, dtype=np.uint8)) % 4
    kept = out[~mask_del]
    ins_pos = np.nonzero(ins[~mask_del])[0]
    if len(ins_pos):
        kept = np.insert(kept, ins_pos + 1, rng.integers(0, 4, size=len(ins_pos), dtype=np.uint8))
    return np.ascontiguousarray(kept).tobytes()


def gen_two_hap_sets(rng, n_sets, depth, qlen):
    sets = []
    for _ in range(n_sets):
        a = rng.integers(0, 4, size=qlen, dtype=np.uint8)
        b = a.copy()
        pos = np.arange(250, qlen, 500) + rng.integers(-100, 100, size=len(range(250, qlen, 500)))
        pos = pos[(pos >= 0) & (pos < qlen)]
        b[pos] = (b[pos] + rng.integers(1, 4, size=len(pos), dtype=np.uint8)) % 4
        cut = int(rng.integers(qlen // 4, 3 * qlen // 4))
        b = np.concatenate([b[:cut], b[cut + 3:]])
        sets.append([noisy(rng, a if i % 2 == 0 else b) for i in range(depth)])
    return sets


class Batch:
    """The batch arguments, built once and reused by every call."""

    def __init__(self, sets, max_n_cons, out_msa):
        self.L = L = abpoa_amd.lib()
        L.abpoa_init_para.restype = ctypes.c_void_p
        L.abpoa_post_set_para.argtypes = [ctypes.c_void_p]
        L.abpoa_amd_msa_batch.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
            ctypes.POINTER(ctypes.POINTER(ctypes.c_int)),
            ctypes.POINTER(ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
            abpoa_amd.CONS_CB, ctypes.c_void_p, ctypes.c_int]
        self.para = L.abpoa_init_para()
        p = ctypes.cast(self.para, ctypes.POINTER(ParaT)).contents
        p.max_n_cons = max_n_cons
        if out_msa:
            p.out_msa = 1
            p.out_cons = 1
        L.abpoa_post_set_para(self.para)
        self.out_msa = out_msa
        self.n = len(sets)
        self.nseqs = (ctypes.c_int * self.n)(*[len(s) for s in sets])
        self.keep = []
        lens_top, ptr_top = [], []
        for s in sets:
            lens = (ctypes.c_int * len(s))(*[len(r) for r in s])
            bufs = [ctypes.create_string_buffer(r, len(r)) for r in s]
            ptrs = (ctypes.POINTER(ctypes.c_uint8) * len(s))(
                *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
            self.keep.append((lens, bufs, ptrs))
            lens_top.append(lens)
            ptr_top.append(ptrs)
        self.lens = (ctypes.POINTER(ctypes.c_int) * self.n)(*lens_top)
        self.seqs = (ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)) * self.n)(*ptr_top)

    def call(self, cb, threads):
        rc = self.L.abpoa_amd_msa_batch(self.para, self.n, self.nseqs, self.lens, self.seqs,
                                        cb, None, threads)
        assert rc == 0


def checksum_cb(acc, out_msa):
    @abpoa_amd.CONS_CB
    def cb(idx, cons_p, _user):
        c = cons_p.contents
        crc = zlib.crc32(b"%d %d %d" % (c.n_cons, c.n_seq, c.msa_len if out_msa else 0))
        for ci in range(c.n_cons):
            ln, ns = c.cons_len[ci], c.clu_n_seq[ci]
            crc = zlib.crc32(b"%d %d" % (ln, ns), crc)
            crc = zlib.crc32(ctypes.string_at(c.cons_base[ci], ln), crc)
            for arr in (c.cons_node_ids[ci], c.cons_cov[ci], c.cons_phred_score[ci]):
                crc = zlib.crc32(ctypes.string_at(arr, 4 * ln), crc)
            crc = zlib.crc32(ctypes.string_at(c.clu_read_ids[ci], 4 * ns), crc)
        if out_msa and c.msa_len > 0:
            for i in range(c.n_seq + c.n_cons):
                crc = zlib.crc32(ctypes.string_at(c.msa_base[i], c.msa_len), crc)
        acc[idx] = (crc, c.n_cons)
    return cb


TIMING_RE = re.compile(r"rounds ([\d.]+)s .* cons ([\d.]+)s \(dl ([\d.]+)s\)")


def timed_call(batch, on, cb, threads):
    """One call with fd 2 captured: (wall s, rounds s, cons s, dl s, stats)."""
    if on:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    abpoa_amd.reset_cons_stats()
    abpoa_amd.reset_msa_stats()
    abpoa_amd.reset_multicons_stats()
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            t0 = time.perf_counter()
            batch.call(cb, threads)
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        text = tf.read().decode(errors="replace")
    os.environ.pop(SWITCH, None)
    m = TIMING_RE.search(text)
    rounds, cons, dl = (float(x) for x in m.groups()) if m else (float("nan"),) * 3
    return wall, rounds, cons, dl, abpoa_amd.get_cons_stats(), abpoa_amd.get_msa_stats(), \
        abpoa_amd.get_multicons_stats()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", type=int, default=250)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--qlen", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--max-n-cons", type=int, default=2)
    ap.add_argument("--out-msa", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20240)
    args = ap.parse_args()

    os.environ["ABPOA_AMD_TIMING"] = "1"
    t0 = time.perf_counter()
    sets = gen_two_hap_sets(np.random.default_rng(args.seed), args.sets, args.depth, args.qlen)
    print("# %d sets x %d reads x %d bp, two haplotypes, max_n_cons %d, out_msa %d, %d host threads "
          "(generated in %.1f s)" % (args.sets, args.depth, args.qlen, args.max_n_cons,
                                     int(args.out_msa), args.threads, time.perf_counter() - t0))
    batch = Batch(sets, args.max_n_cons, args.out_msa)
    null_cb = abpoa_amd.CONS_CB()

    print("%-10s %8s %7s %6s %8s %10s %15s %15s %14s %10s   %s" % (
        "call", "rounds s", "cons s", "dl s", "wall s", "kernel ms", "cons D2H B", "MSA D2H B",
        "stage D2H B", "cand/set", "device/host/fallback"))

    def row(name, r):
        wall, rounds, cons, dl, cs, ms, mc = r
        kern = (cs["kernel_ns"] + ms["kernel_ns"]) / 1e6
        cand = "%.1f" % (mc["cand_cols"] / mc["device_sets"]) if mc["device_sets"] else "-"
        print("%-10s %8.2f %7.2f %6.2f %8.3f %10.2f %15d %15d %14d %10s   %d / %d / %d" % (
            name, rounds, cons, dl, wall, kern, cs["d2h_bytes"], ms["d2h_bytes"],
            mc["d2h_bytes"] if mc["d2h_bytes"] else cs["d2h_bytes"], cand,
            cs["device_sets"], cs["host_sets"], cs["fallback_sets"]))
        sys.stdout.flush()

    for on in (False, True):
        row("warm-" + ("on" if on else "off"), timed_call(batch, on, null_cb, args.threads))
    for k in range(args.calls):
        for on in (False, True):
            row("%s-%d" % ("on" if on else "off", k), timed_call(batch, on, null_cb, args.threads))

    sums = {}
    for on in (False, True):
        acc = [None] * args.sets
        r = timed_call(batch, on, checksum_cb(acc, args.out_msa), args.threads)
        row("crc-" + ("on" if on else "off"), r)
        sums[on] = acc
    n_cons = [x[1] for x in sums[True]]
    same = sums[True] == sums[False]
    print("# checksums over every result field: %s (%d sets; consensus sequences per set: %s)" % (
        "IDENTICAL" if same else "DIFFERENT", args.sets,
        ", ".join("%d x %d" % (n_cons.count(k), k) for k in sorted(set(n_cons)))))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
