"""The convex DP kernel's fast instantiation against the generic one (-m gpu).

cg_global_mw_kernel<S, FAST> hard-codes global mode, banding, no path scores
and the full ring depth, reads the row CSR with scalar loads and loads the
band state of its skip-edge targets at the top of the row. The host picks it
per launch; ABPOA_AMD_DP_GENERIC=1 forces the generic instantiation in the
same build. Every output byte must be the same either way, so the GPU binary
runs under both settings and is compared byte for byte with the CPU oracle
(consensus and -r1 rows; the row-column MSA walks every read's CIGAR):

  - deep short sets at 13 % error: rows with more than MW_NPF predecessors
    and out-edges and far out-edges, int16 and (scaled matrix) int32;
  - two reads of 1-3 bases: 3-5 rows, the rolled loads' clamps, first and
    last row;
  - unbanded, local, extension with z-drop and ABPOA_AMD_DP_RING=1, which
    must all select the generic instantiation, and still match;
  - a band wider than a 512-cell ring slot;
  - the resident batch driver, where the fold kernel writes the CSR.
"""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT, GPU_BIN, run_stdout

pytestmark = pytest.mark.gpu

INT32_SCALED = ["-M", "90", "-X", "180", "-O", "180,1080", "-E", "90,45"]


@pytest.fixture(scope="module")
def gpu_bin():
    assert os.path.exists(GPU_BIN), "abpoa_amd not built (run __graft_entry__.build())"
    return GPU_BIN


def _synth(path, seed, length, depth, noisy=False):
    cmd = [sys.executable, os.path.join(ROOT, "tests", "make_synth.py"), str(path),
           "--seed", str(seed), "--len", str(length), "--depth", str(depth)]
    if noisy:  # 13 % instead of the default 10 %
        cmd += ["--sub", "0.06", "--del", "0.04", "--ins", "0.03"]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def _same_both_ways(gpu_bin, cputest_bin, oracle_env, fa, opts, extra_env=None):
    for extra in ([], ["-r1"]):
        cpu = run_stdout([cputest_bin, str(fa)] + opts + extra, env=oracle_env)
        assert cpu, "oracle produced no output for %r" % (opts + extra,)
        outs = {}
        for generic in (None, "1"):
            env = dict(os.environ)
            env.pop("ABPOA_AMD_DP_GENERIC", None)
            env.pop("ABPOA_AMD_DP_RING", None)
            env.update(extra_env or {})
            if generic:
                env["ABPOA_AMD_DP_GENERIC"] = generic
            outs[generic] = run_stdout([gpu_bin, str(fa)] + opts + extra, env=env)
            assert outs[generic] == cpu, \
                "GPU/oracle divergence opts=%r generic=%r" % (opts + extra, generic)
        assert outs[None] == outs["1"]


@pytest.fixture(scope="module")
def deep_fa(tmp_path_factory):
    fa = tmp_path_factory.mktemp("fast") / "deep.fa"
    _synth(fa, 81, 400, 16, noisy=True)
    return fa


@pytest.mark.parametrize("opts", [[], INT32_SCALED], ids=["int16", "int32-scaled"])
def test_deep_short(gpu_bin, cputest_bin, oracle_env, deep_fa, opts):
    """16 reads x 400 bases at 13 % error; 400 x 90 > INT16_MAX forces int32."""
    _same_both_ways(gpu_bin, cputest_bin, oracle_env, deep_fa, opts)


@pytest.mark.parametrize("reads", [("A", "A"), ("AC", "AG"), ("ACG", "ATG")],
                         ids=["1bp", "2bp", "3bp"])
def test_tiny_graphs(gpu_bin, cputest_bin, oracle_env, tmp_path, reads):
    """n_rows of 3 to 5: every rolled index is clamped on some row."""
    fa = tmp_path / "tiny.fa"
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    _same_both_ways(gpu_bin, cputest_bin, oracle_env, fa, [])


def test_fast_eligibility():
    """The predicate both host paths use to pick the instantiation."""
    sys.path.insert(0, ROOT)
    import abpoa_amd
    L = abpoa_amd.lib()
    f = L.abamd_cg_fast_eligible
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4
    ring_max = 10
    assert f(0, 1, 0, ring_max) == 1
    assert f(0, 0, 0, ring_max) == 0      # unbanded
    assert f(1, 1, 0, ring_max) == 0      # local
    assert f(2, 1, 0, ring_max) == 0      # extension
    assert f(0, 1, 1, ring_max) == 0      # path scores
    assert f(0, 1, 0, 1) == 0             # ABPOA_AMD_DP_RING=1
    assert f(0, 1, 0, ring_max - 1) == 0
    g = L.abamd_dp_force_generic
    g.restype = ctypes.c_int
    saved = os.environ.pop("ABPOA_AMD_DP_GENERIC", None)
    try:
        assert g() == 0
        os.environ["ABPOA_AMD_DP_GENERIC"] = "1"
        assert g() == 1
        os.environ["ABPOA_AMD_DP_GENERIC"] = "0"
        assert g() == 0
    finally:
        os.environ.pop("ABPOA_AMD_DP_GENERIC", None)
        if saved is not None:
            os.environ["ABPOA_AMD_DP_GENERIC"] = saved


@pytest.mark.parametrize("opts,env", [(["-b", "-1"], None), (["-m1"], None),
                                      (["-m2", "-z", "100"], None),
                                      ([], {"ABPOA_AMD_DP_RING": "1"})],
                         ids=["unbanded", "local", "extend-zdrop", "ring1"])
def test_generic_only_modes(gpu_bin, cputest_bin, oracle_env, deep_fa, opts, env):
    """Not eligible for the fast instantiation (test_fast_eligibility): the
    default setting must run the generic kernel here and match the oracle."""
    _same_both_ways(gpu_bin, cputest_bin, oracle_env, deep_fa, opts, extra_env=env)


def test_band_wider_than_slot(gpu_bin, cputest_bin, oracle_env, tmp_path):
    """600 bases, -b 300: 2w + 1 = 613 cells, clipped to the query, is wider
    than a 512-cell slot: two superchunks per row, arena gathers."""
    fa = tmp_path / "wide.fa"
    _synth(fa, 82, 600, 12)
    _same_both_ways(gpu_bin, cputest_bin, oracle_env, fa, ["-b", "300"])


def test_resident_batch_fast_and_generic(gpu_bin, tmp_path):
    """6 sets x 12 reads x 400 bases through the resident batch driver (the
    fold kernel writes the CSR the scalar loads read): both settings agree
    set for set, and with the sequential CLI."""
    sys.path.insert(0, ROOT)
    import importlib
    import numpy as np
    import abpoa_amd
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(808)
    sets = bench.gen_sets(rng, 6, depth=12, qlen=400)
    saved = os.environ.pop("ABPOA_AMD_DP_GENERIC", None)
    try:
        fast = abpoa_amd.msa_batch_consensus(sets, n_threads=2)
        os.environ["ABPOA_AMD_DP_GENERIC"] = "1"
        generic = abpoa_amd.msa_batch_consensus(sets, n_threads=2)
    finally:
        os.environ.pop("ABPOA_AMD_DP_GENERIC", None)
        if saved is not None:
            os.environ["ABPOA_AMD_DP_GENERIC"] = saved
    assert len(fast) == len(sets)
    for i, s in enumerate(sets):
        assert fast[i] == generic[i], "instantiation changed the consensus of set %d" % i
        fa = tmp_path / ("s%d.fa" % i)
        with open(fa, "w") as f:
            for r_i, r in enumerate(s):
                f.write(">r%d\n%s\n" % (r_i, "".join("ACGT"[b] for b in r)))
        out = run_stdout([gpu_bin, str(fa)]).decode()
        assert fast[i] == "".join(out.splitlines()[1:]), "batch/CLI mismatch on set %d" % i
