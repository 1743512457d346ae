"""Row-column MSA from the batched driver, CPU parity (no GPU needed).

abpoa_amd_batchtest -r1 / -r2 runs abpoa_amd_msa_batch with abpt->out_msa set
and the oracle injected through the dispatch seam, and prints each set's MSA
rows after its ">set_N" consensus record. The rows must equal, in order and
with names ignored, the sequence lines of the sequential CLI
(abpoa_amd_cputest -r1 / -r2) on the same file and the committed reference
outputs for seq.fa, and must not depend on the pipeline shape."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT, CSRC, GOLDEN, CPUTEST_BIN as CPU_BIN, ORACLE_SO, run_stdout
from test_batch_cpu import _gen_sets

BATCH_BIN = os.path.join(CSRC, "abpoa_amd_batchtest")
CPU_LIB = os.path.join(CSRC, "libabpoa_amd_cputest.so")


def _env(cputest_bin, groups=None):
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    if groups is not None:
        env["ABPOA_AMD_GROUPS"] = groups
    return env


def _records(out):
    """[(consensus, [msa rows])] per ">set_N" record of the tool's output."""
    recs = []
    for rec in out.decode().split(">")[1:]:
        lines = rec.split("\n")
        assert lines[0].startswith("set_") and lines[-1] == ""
        recs.append((lines[1], lines[2:-1]))
    return recs


def _seq_lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith(">")]


@pytest.mark.parametrize("opt", ["-r1", "-r2"])
def test_batch_msa_rows_match_cli(cputest_bin, tmp_path, opt):
    paths = _gen_sets(tmp_path) + [os.path.join(GOLDEN, "seq.fa")]
    outs = {g: subprocess.run([BATCH_BIN, opt] + paths, env=_env(cputest_bin, g), check=True,
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            for g in ("1", "3")}
    assert outs["1"] == outs["3"], "batch MSA differs across pipeline group counts"
    plain = subprocess.run([BATCH_BIN] + paths, env=_env(cputest_bin, "1"), check=True,
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    recs = _records(outs["1"])
    assert len(recs) == len(paths)
    # the consensus records are those of the run without the option
    assert [c for c, _rows in recs] == [c for c, _rows in _records(plain)]
    assert all(rows == [] for _c, rows in _records(plain))
    for i, p in enumerate(paths):
        cli = _seq_lines(run_stdout([CPU_BIN, opt, p], env=_env(cputest_bin)).decode())
        cons, rows = recs[i]
        assert rows == cli, "batch/CLI %s rows differ on set %d" % (opt, i)
        n_reads = sum(1 for ln in open(p) if ln.startswith(">"))
        assert len(rows) == n_reads + (1 if opt == "-r2" else 0)
        assert len({len(r) for r in rows}) == 1 and set("".join(rows)) <= set("ACGTN-")
        if opt == "-r2":
            assert rows[-1].replace("-", "") == cons
    # the committed reference output for seq.fa
    golden = open(os.path.join(GOLDEN, "expected_seq_r%s.txt" % opt[-1])).read()
    assert recs[-1][1] == _seq_lines(golden)


def test_msa_stats_api_cpu_library(cputest_bin, monkeypatch):
    """The CPU test library exports the MSA stats symbols and reports zeros;
    abpoa_amd.get_msa_stats() works against it."""
    h = ctypes.CDLL(CPU_LIB)
    v = [ctypes.c_uint64(7) for _ in range(5)]
    h.abpoa_amd_reset_msa_stats()
    h.abpoa_amd_get_msa_stats(*[ctypes.byref(x) for x in v])
    assert [x.value for x in v] == [0, 0, 0, 0, 0]
    # NULL pointers are allowed
    h.abpoa_amd_get_msa_stats.argtypes = [ctypes.c_void_p] * 5
    h.abpoa_amd_get_msa_stats(None, None, None, None, None)

    import sys
    sys.path.insert(0, ROOT)
    import abpoa_amd
    monkeypatch.setenv("ABPOA_AMD_LIB", CPU_LIB)
    monkeypatch.setattr(abpoa_amd, "_lib", None)
    abpoa_amd.reset_msa_stats()
    assert abpoa_amd.get_msa_stats() == {
        "device_sets": 0, "host_sets": 0, "fallback_sets": 0, "d2h_bytes": 0, "kernel_ns": 0}
