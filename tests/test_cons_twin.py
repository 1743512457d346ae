"""Phased flat consensus (the device consensus kernel's shared body) vs the
pointer-graph consensus, on CPU.

abpoa_amd_constwin replays oracle CIGARs into the pointer graph and the flat
device-layout graph and, after EVERY read, runs abamd_flat_cons_phased (one
lane) over the flat graph + its topological order, builds an abpoa_cons_t
with abamd_cons_from_path and compares every field (n_cons, n_seq, cons_len,
node ids, bases, coverage, phred, clu_n_seq, clu_read_ids) against
abpoa_generate_consensus, plus the queue-based flat core as second witness.

Also checks the consensus-stage stats API against the CPU test library."""
import ctypes
import os
import subprocess

import cons_cases
from conftest import ROOT, CSRC, GOLDEN, ORACLE_SO

TWIN = os.path.join(CSRC, "abpoa_amd_constwin")
CPU_LIB = os.path.join(CSRC, "libabpoa_amd_cputest.so")


def _run(fa, extra=()):
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    out = subprocess.run([TWIN, fa] + list(extra), env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, "%s %s: %s" % (fa, extra, out.stderr.decode()[-500:])
    assert b"cons twin OK" in out.stdout


def test_cons_twin_golden(cputest_bin):
    for fa in ("seq.fa", "test.fa", "heter.fa", "3alleles.fa"):
        _run(os.path.join(GOLDEN, fa))
        _run(os.path.join(GOLDEN, fa), ["-r1"])


def test_cons_twin_synthetic(cputest_bin, tmp_path):
    # the shapes of test_fold_twin.py::test_twin_synthetic
    for seed, length, depth in ((1, 300, 12), (2, 900, 20), (3, 1800, 30), (4, 4000, 40),
                                (5, 600, 80)):
        fa = str(tmp_path / ("s%d.fa" % seed))
        subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), fa,
                        "--seed", str(seed), "--len", str(length), "--depth", str(depth)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        _run(fa)
        _run(fa, ["-r1"])


def test_cons_twin_tie_stress(cputest_bin, tmp_path):
    """Equal-weight, equal-score out-edges at every variant site (and at SRC)
    and row counts on both sides of the 64-row staging step."""
    for name, reads in cons_cases.all_sets():
        fa = str(tmp_path / (name + ".fa"))
        cons_cases.write_fasta(fa, reads)
        _run(fa)
        _run(fa, ["-r1"])


def test_cons_stats_api_cpu_library(cputest_bin, monkeypatch):
    """The CPU test library exports the consensus-stage stats symbols and
    reports zeros; abpoa_amd.get_cons_stats() works against it."""
    h = ctypes.CDLL(CPU_LIB)
    v = [ctypes.c_uint64(7) for _ in range(5)]
    h.abpoa_amd_reset_cons_stats()
    h.abpoa_amd_get_cons_stats(*[ctypes.byref(x) for x in v])
    assert [x.value for x in v] == [0, 0, 0, 0, 0]
    # NULL pointers are allowed
    h.abpoa_amd_get_cons_stats.argtypes = [ctypes.c_void_p] * 5
    h.abpoa_amd_get_cons_stats(None, None, None, None, None)

    import sys
    sys.path.insert(0, ROOT)
    import abpoa_amd
    monkeypatch.setenv("ABPOA_AMD_LIB", CPU_LIB)
    monkeypatch.setattr(abpoa_amd, "_lib", None)
    abpoa_amd.reset_cons_stats()
    assert abpoa_amd.get_cons_stats() == {
        "device_sets": 0, "host_sets": 0, "fallback_sets": 0, "d2h_bytes": 0, "kernel_ns": 0}
