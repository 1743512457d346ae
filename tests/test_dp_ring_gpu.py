"""The convex DP kernel's LDS row ring (-m gpu).

The kernel keeps the H/E1/E2 bands of the last rows in an LDS ring and
gathers near predecessors from it; far predecessors, and rows whose band is
wider than a ring slot, read the arena. Every value must be the one the arena
holds, so the GPU binary is compared byte for byte with the CPU oracle on
identical input (consensus and -r1 rows; the row-column MSA walks every
read's CIGAR), on graphs chosen to take each of those paths and the seams
between them:

  - deep short sets: nearly every row has predecessors several rows back and
    every band fits a slot (int16, and int32 through a scaled score matrix);
  - a deletion and an insertion of 40 bases: edges far longer than the ring;
  - band widths below, at and above the 512-cell slot, and unbanded rows;
  - local and extension mode, which run the same kernel;
  - the resident batch driver, ring on and off (ABPOA_AMD_DP_RING=1).
"""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, GPU_BIN, run_stdout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_bin():
    assert os.path.exists(GPU_BIN), "abpoa_amd not built (run __graft_entry__.build())"
    return GPU_BIN


def _synth(path, seed, length, depth):
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "make_synth.py"), str(path),
                    "--seed", str(seed), "--len", str(length), "--depth", str(depth)],
                   check=True, stderr=subprocess.DEVNULL)


def _same_as_oracle(gpu_bin, cputest_bin, oracle_env, fa, opts):
    for extra in ([], ["-r1"]):
        cpu = run_stdout([cputest_bin, str(fa)] + opts + extra, env=oracle_env)
        assert cpu, "oracle produced no output for %r" % (opts + extra,)
        for ring in (None, "1"):
            env = dict(os.environ)
            env.pop("ABPOA_AMD_DP_RING", None)
            if ring:
                env["ABPOA_AMD_DP_RING"] = ring
            gpu = run_stdout([gpu_bin, str(fa)] + opts + extra, env=env)
            assert gpu == cpu, "GPU/oracle divergence opts=%r ring=%r" % (opts + extra, ring)


@pytest.fixture(scope="module")
def deep_short_fa(tmp_path_factory):
    fa = tmp_path_factory.mktemp("ring") / "deep.fa"
    _synth(fa, 61, 400, 80)
    return fa


# -M9 is the scoring of the suite's forced-int32 input; at 400 bases its score
# bound (400 x 9) still fits int16, so the last case scales the default
# scoring by 45 (400 x 90 > INT16_MAX): the same alignments through the int32
# instantiation of the kernel and its twice-as-large ring slots.
@pytest.mark.parametrize("opts", [[], ["-M9"],
                                  ["-M", "90", "-X", "180", "-O", "180,1080", "-E", "90,45"]],
                         ids=["int16", "M9", "int32-scaled"])
def test_deep_short(gpu_bin, cputest_bin, oracle_env, deep_short_fa, opts):
    """--len 400 --depth 80: far predecessors on nearly every row, all bands fit."""
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, deep_short_fa, opts)


def test_edges_longer_than_ring(gpu_bin, cputest_bin, oracle_env, tmp_path):
    """12 reads of a 600-base reference with scattered substitutions; four
    lack the same 40 bases and four carry the same 40-base insertion, so the
    graph has edges that skip far more rows than the ring holds."""
    rng = random.Random(5)
    ref = "".join(rng.choice("ACGT") for _ in range(600))
    ins = "".join(rng.choice("ACGT") for _ in range(40))

    def subst(s):
        return "".join(rng.choice([c for c in "ACGT" if c != ch]) if rng.random() < 0.03 else ch
                       for ch in s)

    reads = []
    for i in range(12):
        if i % 3 == 1:
            s = ref[:250] + ref[290:]
        elif i % 3 == 2:
            s = ref[:400] + ins + ref[400:]
        else:
            s = ref
        reads.append(subst(s))
    fa = tmp_path / "indel.fa"
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, fa, [])


@pytest.fixture(scope="module")
def band_fa(tmp_path_factory):
    fa = tmp_path_factory.mktemp("ring") / "band.fa"
    _synth(fa, 62, 1500, 20)
    return fa


# w = b + 0.01 * qlen (about 15 here): 2w = 230 lies below the 512-cell slot,
# 2w = 512 at it (a row's band is 2w + 1 plus the spread of its predecessors'
# maxima, so rows that fit and rows that do not alternate), 2w = 830 above it
# (two 512-thread superchunks per row; rows clipped at the ends still fit).
@pytest.mark.parametrize("b", [100, 241, 400])
def test_band_around_slot_width(gpu_bin, cputest_bin, oracle_env, band_fa, b):
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, band_fa, ["-b", str(b)])


@pytest.mark.parametrize("length", [300, 700])
def test_unbanded(gpu_bin, cputest_bin, oracle_env, tmp_path, length):
    """-b -1: every row spans the whole query; 300 fits a slot, 700 does not."""
    fa = tmp_path / "u.fa"
    _synth(fa, 63, length, 20)
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, fa, ["-b", "-1"])


@pytest.mark.parametrize("opts", [["-m1"], ["-m2"], ["-m2", "-z", "100"]],
                         ids=["local", "extend", "extend-zdrop"])
def test_local_and_extension(gpu_bin, cputest_bin, oracle_env, deep_short_fa, opts):
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, deep_short_fa, opts)


def test_resident_batch_ring_on_off(gpu_bin, tmp_path):
    """8 sets x 30 reads, 500..1500 bases, through the resident batch driver:
    ring at its default depth and at 1 must agree set for set, and with the
    sequential CLI."""
    sys.path.insert(0, ROOT)
    import importlib
    import numpy as np
    import abpoa_amd
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(606)
    sets = []
    for qlen in (500, 640, 790, 930, 1070, 1210, 1360, 1500):
        sets += bench.gen_sets(rng, 1, depth=30, qlen=qlen)
    saved = os.environ.pop("ABPOA_AMD_DP_RING", None)
    try:
        ring = abpoa_amd.msa_batch_consensus(sets, n_threads=2)
        os.environ["ABPOA_AMD_DP_RING"] = "1"
        prev_only = abpoa_amd.msa_batch_consensus(sets, n_threads=2)
    finally:
        os.environ.pop("ABPOA_AMD_DP_RING", None)
        if saved is not None:
            os.environ["ABPOA_AMD_DP_RING"] = saved
    assert len(ring) == len(sets)
    for i, s in enumerate(sets):
        assert ring[i] == prev_only[i], "ring depth changed the consensus of set %d" % i
        fa = tmp_path / ("s%d.fa" % i)
        with open(fa, "w") as f:
            for r_i, r in enumerate(s):
                f.write(">r%d\n%s\n" % (r_i, "".join("ACGT"[b] for b in r)))
        out = run_stdout([gpu_bin, str(fa)]).decode()
        assert ring[i] == "".join(out.splitlines()[1:]), "batch/CLI mismatch on set %d" % i
