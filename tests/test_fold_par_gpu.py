"""Lane-parallel graph mutation walk on the GPU (abamd_fold_par.inc inside
abamd_fold_round_kernel).

abpoa_amd_foldgpu -p drives a 64-lane validation kernel through the walk, one
launch per read, and compares the whole device graph with the host twin after
every read. The resident batch driver must then give byte-identical consensus,
coverage and rows with the parallel walk (default) and with the serial lane-0
walk (ABPOA_AMD_SERIAL_FOLD=1), take the parallel path for every fold, and
never fall back."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)

FOLDGPU = os.path.join(ROOT, "abpoa_amd", "csrc", "abpoa_amd_foldgpu")


@pytest.fixture(scope="module")
def depth80_fa(tmp_path_factory):
    """600 bp x 80 reads: two read-id words per edge."""
    fa = str(tmp_path_factory.mktemp("foldpar") / "d80.fa")
    subprocess.run(["python3", os.path.join(ROOT, "tests", "make_synth.py"), fa,
                    "--seed", "5", "--len", "600", "--depth", "80"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return fa


def _foldgpu_p(fa):
    out = subprocess.run([FOLDGPU, fa, "-p"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-500:]
    assert b"device fold OK" in out.stdout and b"parallel walk, fallbacks 0" in out.stdout


@pytest.mark.parametrize("fa", ["seq.fa", "fgt.fa"])
def test_validation_kernel_golden(fa):
    _foldgpu_p(os.path.join(GOLDEN, fa))


def test_validation_kernel_depth80(depth80_fa):
    _foldgpu_p(depth80_fa)


def _read_fa(fa):
    reads = []
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            reads.append([])
        elif line:
            reads[-1].append(line)
    return [bytes("ACGT".index(c) for c in "".join(p).upper()) for p in reads]


def _run(sets, serial):
    import abpoa_amd
    saved = os.environ.get("ABPOA_AMD_SERIAL_FOLD")
    if serial:
        os.environ["ABPOA_AMD_SERIAL_FOLD"] = "1"
    else:
        os.environ.pop("ABPOA_AMD_SERIAL_FOLD", None)
    try:
        abpoa_amd.reset_fold_stats()
        res = abpoa_amd.msa_batch_results(sets, n_threads=2, out_msa=True, out_cons=True)
        stats = abpoa_amd.get_fold_stats()
    finally:
        if saved is None:
            os.environ.pop("ABPOA_AMD_SERIAL_FOLD", None)
        else:
            os.environ["ABPOA_AMD_SERIAL_FOLD"] = saved
    return res, stats


def test_resident_parallel_matches_serial(depth80_fa):
    bench = importlib.import_module("bench")
    sets = bench.gen_sets(np.random.default_rng(2024), 6, depth=12, qlen=600)
    sets.append(_read_fa(depth80_fa))
    n_folds = sum(len(s) for s in sets)   # one fold job per read, the first included

    par, st = _run(sets, serial=False)
    assert st == {"parallel_folds": n_folds, "fallback_folds": 0, "serial_folds": 0}, st
    ser, ss = _run(sets, serial=True)
    assert ss == {"parallel_folds": 0, "fallback_folds": 0, "serial_folds": n_folds}, ss

    assert len(par) == len(ser) == len(sets)
    for i, (x, y) in enumerate(zip(par, ser)):
        assert x.keys() == y.keys()
        for k in ("cons", "cov", "msa", "msa_len"):
            assert k in x
        for k in x:
            assert x[k] == y[k], "set %d field %s differs between the walks" % (i, k)
