"""The affine and linear multi-wave DP kernels (-m gpu).

Both kernels share one frame (band steering, row argmax, running best with
z-drop, arena reservation, backtrack) around their own recurrence. The GPU
binary is compared byte for byte with the CPU oracle on identical input
(consensus and -r1 rows; the row-column MSA walks every read's CIGAR), for
both gap modes on inputs chosen to take each path of that frame:

  - a deep short set: far predecessors on nearly every row, every band fits
    the LDS previous-row cache (int16, and int32 through scaled scoring);
  - local and extension mode, and extension mode with a z-drop that fires;
  - band widths below, at and above the 512-thread superchunk: the widest
    takes two superchunks per row (carry across superchunks, and the arena
    gather of a previous row that did not fit the cache);
  - unbanded rows that fit the cache and rows that do not.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, GPU_BIN, run_stdout

pytestmark = pytest.mark.gpu

# default scoring is -M 2 -X 4; the scaled set multiplies it by 45, so that
# 400 bases x 90 > INT16_MAX and the int32 instantiations run the same
# alignments
GAPS = {"affine": ["-O", "4", "-E", "2"], "linear": ["-O", "0", "-E", "2"]}
GAPS_X45 = {"affine": ["-M", "90", "-X", "180", "-O", "180", "-E", "90"],
            "linear": ["-M", "90", "-X", "180", "-O", "0", "-E", "90"]}
GAP_IDS = sorted(GAPS)


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
        gpu = run_stdout([gpu_bin, str(fa)] + opts + extra)
        assert gpu == cpu, "GPU/oracle divergence opts=%r" % (opts + extra,)


@pytest.fixture(scope="module")
def deep_short_fa(tmp_path_factory):
    fa = tmp_path_factory.mktemp("gap") / "deep.fa"
    _synth(fa, 71, 400, 80)
    return fa


@pytest.mark.parametrize("gap", GAP_IDS)
@pytest.mark.parametrize("scoring", ["int16", "int32-scaled"])
def test_deep_short(gpu_bin, cputest_bin, oracle_env, deep_short_fa, gap, scoring):
    """--len 400 --depth 80: far predecessors on nearly every row, all bands fit."""
    opts = GAPS[gap] if scoring == "int16" else GAPS_X45[gap]
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, deep_short_fa, opts)


@pytest.mark.parametrize("gap", GAP_IDS)
@pytest.mark.parametrize("mode", [["-m1"], ["-m2"], ["-m2", "-z", "5"]],
                         ids=["local", "extend", "extend-zdrop"])
def test_local_and_extension(gpu_bin, cputest_bin, oracle_env, deep_short_fa, gap, mode):
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, deep_short_fa, GAPS[gap] + mode)


@pytest.mark.parametrize("gap", GAP_IDS)
def test_zdrop_fires_on_this_input(cputest_bin, oracle_env, deep_short_fa, gap):
    """The z-drop cases above mean something only if -z 5 really ends
    alignments early here: the oracle's rows must differ from those without."""
    base = [cputest_bin, str(deep_short_fa)] + GAPS[gap]
    plain = run_stdout(base + ["-m2", "-r1"], env=oracle_env)
    dropped = run_stdout(base + ["-m2", "-z", "5", "-r1"], env=oracle_env)
    assert plain and dropped
    assert dropped != plain, "-z 5 does not fire on the deep set (%s)" % gap


@pytest.mark.parametrize("gap", GAP_IDS)
def test_extension_zdrop_int32(gpu_bin, cputest_bin, oracle_env, deep_short_fa, gap):
    """-z 100 against scores scaled by 45 fires as well, in the int32 kernels."""
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, deep_short_fa,
                    GAPS_X45[gap] + ["-m2", "-z", "100"])


@pytest.fixture(scope="module")
def band_fa(tmp_path_factory):
    fa = tmp_path_factory.mktemp("gap") / "band.fa"
    _synth(fa, 72, 1500, 20)
    return fa


# w = b + 0.01 * qlen (about 15 here): 2w = 230 lies below the 512-thread
# superchunk, 2w = 512 at it (a row's band is 2w + 1 plus the spread of its
# predecessors' maxima, so rows that fit and rows that do not alternate),
# 2w = 830 above it (two superchunks per row; rows clipped at the ends fit).
@pytest.mark.parametrize("gap", GAP_IDS)
@pytest.mark.parametrize("b", [100, 241, 400])
def test_band_around_superchunk_width(gpu_bin, cputest_bin, oracle_env, band_fa, gap, b):
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, band_fa, GAPS[gap] + ["-b", str(b)])


@pytest.fixture(scope="module", params=[300, 700])
def unbanded_fa(request, tmp_path_factory):
    fa = tmp_path_factory.mktemp("gap") / ("u%d.fa" % request.param)
    _synth(fa, 73, request.param, 20)
    return fa


@pytest.mark.parametrize("gap", GAP_IDS)
def test_unbanded(gpu_bin, cputest_bin, oracle_env, unbanded_fa, gap):
    """-b -1: every row spans the whole query; 300 fits the cache, 700 does not."""
    _same_as_oracle(gpu_bin, cputest_bin, oracle_env, unbanded_fa, GAPS[gap] + ["-b", "-1"])
