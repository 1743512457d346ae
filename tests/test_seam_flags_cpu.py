"""Effect guards for tests/test_seam_gpu.py and the GPU flag cases of
tests/test_gpu_parity.py, in the manner of test_zdrop_fires_on_this_input: a
flag case means something only if, on the input it runs on, the oracle's
output with the flag differs from its output without it. Runs on the CPU."""
import os

import pytest

from conftest import run_stdout
import seam_cases as sc


@pytest.fixture(scope="module")
def s91(tmp_path_factory):
    return sc.synth13(tmp_path_factory.mktemp("flags") / "s91.fa")


def _rows(cputest_bin, oracle_env, fa, opts):
    out = run_stdout([cputest_bin, str(fa)] + opts + ["-r1"], env=oracle_env)
    assert out
    return out


@pytest.mark.parametrize("flags", [["-R"], ["-J"], ["-R", "-J"]], ids=lambda f: "".join(f))
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_gap_placement_changes_rows(cputest_bin, oracle_env, s91, gap, flags):
    plain = _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap])
    assert _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap] + flags) != plain


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_path_scores_change_rows(cputest_bin, oracle_env, gap, width):
    scoring = sc.GAPS[gap] if width == 16 else sc.GAPS_X45[gap]
    plain = _rows(cputest_bin, oracle_env, sc.SYNTH13_SEED1, scoring)
    assert _rows(cputest_bin, oracle_env, sc.SYNTH13_SEED1, scoring + ["-G"]) != plain


@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_extension_changes_rows(cputest_bin, oracle_env, s91, gap):
    """-e 5 -m2: the bonus is never read, but the case still differs from the
    global one through -m2."""
    plain = _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap])
    assert _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap] + ["-e", "5", "-m2"]) != plain


@pytest.mark.parametrize("width,z", [(16, "5"), (32, "5"), (32, "100")])
@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_zdrop_fires(cputest_bin, oracle_env, s91, gap, width, z):
    """The z-drop cases of test_gap_and_alignment_modes end alignments early
    here: -z 5 at both widths, -z 100 against the x45 scores."""
    scoring = sc.GAPS[gap] if width == 16 else sc.GAPS_X45[gap]
    plain = _rows(cputest_bin, oracle_env, s91, scoring + ["-m2"])
    assert _rows(cputest_bin, oracle_env, s91, scoring + ["-m2", "-z", z]) != plain


@pytest.mark.parametrize("gap", sc.GAP_IDS)
def test_zdrop_100_is_idle_at_int16(cputest_bin, oracle_env, s91, gap):
    """Why -z 5 is there: -z 100 changes nothing at int16 on this input, so
    the int16 extend-z100 seam cases repeat the extension ones."""
    plain = _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap] + ["-m2"])
    assert _rows(cputest_bin, oracle_env, s91, sc.GAPS[gap] + ["-m2", "-z", "100"]) == plain


@pytest.mark.parametrize("opts", [[], ["-r1"]], ids=["cons", "rc-msa"])
def test_restore_changes_output(cputest_bin, oracle_env, tmp_path, opts):
    """-i: the 18 reads aligned into the restored graph of the first 6 give
    other output than the 18 reads alone."""
    dump, rest = sc.restore_inputs(
        tmp_path, lambda first: run_stdout([cputest_bin, first, "-r4"], env=oracle_env))
    alone = run_stdout([cputest_bin, rest] + opts, env=oracle_env)
    assert alone and run_stdout([cputest_bin, "-i", dump, rest] + opts, env=oracle_env) != alone


def test_quality_weights_change_output(cputest_bin, oracle_env, tmp_path):
    fq = sc.fastq(tmp_path / "q.fq")
    assert run_stdout([cputest_bin, fq, "-Q", "-r5"], env=oracle_env) != \
        run_stdout([cputest_bin, fq, "-r5"], env=oracle_env)


def test_amb_strand_changes_rows(cputest_bin, oracle_env, s91, tmp_path):
    fa = sc.every_third_reversed(s91, tmp_path / "rc.fa")
    assert _rows(cputest_bin, oracle_env, fa, ["-s"]) != _rows(cputest_bin, oracle_env, fa, [])


def test_long_insertion_input_has_one(tmp_path):
    reads = sc.read_fasta(sc.long_insertion(tmp_path / "ins.fa"))
    assert [len(r) for r in reads] == [120, 720, 720, 1220, 1220, 120]
    assert reads[1][:60] == reads[0][:60] and reads[1][660:] == reads[0][60:]
