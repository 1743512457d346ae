"""bench.py command line: --dump-outputs writes the last timed step's
consensus reproducibly, and a plain run leaves the --full legs alone.

The CPU tests run the benchmark against the CPU test library with the oracle
injected through the dispatch seam; the -m gpu test runs the product library
and must dump exactly what the oracle-injected run dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, CSRC, ORACLE_SO

SHAPE = ["--gpus", "1", "--steps", "2", "--warmup", "1",
         "--sets-per-step", "30", "--depth", "6", "--qlen", "300", "--threads", "2"]
NAMES = ["cons_len", "cons_base", "cons_base_sets", "cons_cov", "cons_cov_sets"]


def _bench(out_dir, extra=(), cpu=True):
    env = dict(os.environ)
    if cpu:
        env["ABPOA_AMD_LIB"] = os.path.join(CSRC, "libabpoa_amd_cputest.so")
        env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SHAPE
                       + ["--dump-outputs", str(out_dir)] + list(extra),
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "expected exactly one JSON line"
    return json.loads(lines[0]), {n: np.load(os.path.join(str(out_dir), n + ".npy")) for n in NAMES}


@pytest.fixture(scope="module")
def cpu_run(cputest_bin, tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("dump_cpu"))


def test_plain_line_and_dump_layout(cpu_run):
    rec, out = cpu_run
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "sets/s" and rec["higher_is_better"] is True
    # the legs that take runs of their own stay behind --full
    assert rec["cpu_baseline"] is None and rec["roofline"]["traffic"] is None
    for a in out.values():
        assert a.dtype in (np.float32, np.float64)
    assert out["cons_len"].shape == (30,)
    assert np.array_equal(out["cons_base_sets"], np.arange(30))
    assert np.array_equal(out["cons_cov_sets"], np.arange(30))
    width = int(out["cons_len"].max())
    assert out["cons_base"].shape == (30, width) and out["cons_cov"].shape == (30, width)
    for i, ln in enumerate(out["cons_len"].astype(int)):
        assert 270 <= ln <= 330
        assert ((out["cons_base"][i, :ln] >= 0) & (out["cons_base"][i, :ln] <= 3)).all()
        assert ((out["cons_cov"][i, :ln] >= 1) & (out["cons_cov"][i, :ln] <= 6)).all()
        assert (out["cons_base"][i, ln:] == -1).all() and (out["cons_cov"][i, ln:] == -1).all()


def test_dump_is_the_last_timed_step(cpu_run):
    """The dump is what the batch driver returns for step warmup+steps-1's
    inputs, and those inputs do not depend on how they were generated."""
    sys.path.insert(0, ROOT)
    import bench
    chunks = bench.gen_step_chunks(None, 0, 2, 30, 6, 300, 4)
    sets = []
    for data, lens in chunks:
        off = np.concatenate([[0], np.cumsum(lens)])
        reads = [data[off[i]:off[i + 1]] for i in range(len(lens))]
        sets += [reads[i:i + 6] for i in range(0, len(reads), 6)]
    env = {"ABPOA_AMD_LIB": os.path.join(CSRC, "libabpoa_amd_cputest.so"),
           "ABPOA_AMD_TEST_ALIGNER_SO": ORACLE_SO}
    code = ("import sys, json, pickle, abpoa_amd; sets = pickle.load(sys.stdin.buffer); "
            "print(json.dumps(abpoa_amd.msa_batch_consensus(sets, n_threads=2)))")
    import pickle
    r = subprocess.run([sys.executable, "-c", code], input=pickle.dumps(sets), cwd=ROOT,
                       env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL, check=True)
    want = json.loads(r.stdout.decode().splitlines()[-1])
    _, out = cpu_run
    got = ["".join("ACGT"[int(b)] for b in out["cons_base"][i, :int(out["cons_len"][i])])
           for i in range(30)]
    assert got == want


def test_dump_repeats(cpu_run, tmp_path):
    _, first = cpu_run
    _, again = _bench(tmp_path / "again")
    for n in NAMES:
        assert np.array_equal(first[n], again[n]), n


def test_dump_sample_fits_budget():
    sys.path.insert(0, ROOT)
    import bench
    rows = bench._dump_rows(1000, 10050 * 4, 16 * 1000 * 1000)
    assert len(rows) == 16 * 1000 * 1000 // (10050 * 4)
    assert np.array_equal(rows, np.unique(rows)) and rows.max() < 1000
    assert np.array_equal(rows, bench._dump_rows(1000, 10050 * 4, 16 * 1000 * 1000))
    assert np.array_equal(bench._dump_rows(10, 100, 16 * 1000 * 1000), np.arange(10))


@pytest.mark.gpu
def test_gpu_dump_matches_oracle(cpu_run, tmp_path):
    """The product library's timed path returns, output for output, what the
    oracle-injected host pipeline returns on the same seeded inputs."""
    _, want = cpu_run
    rec, got = _bench(tmp_path / "gpu", cpu=False)
    assert rec["config"]["total_cells"] > 0, "the GPU hot path did not run"
    for n in NAMES:
        assert np.array_equal(got[n], want[n]), n
