"""The per-round fold check's own comparison, on the CPU
(abpoa_amd_foldroundtwin).

tests/test_fold_round_gpu.py hands abamd_fold_round_check.c what the
production fold kernel wrote, fold by fold. Here the "device" is a second flat
twin advanced by the same serial passes from the oracle's CIGARs, handed over
through the same probe struct. Unchanged it must pass, on the inputs the GPU
cases use; with one thing changed in the copy handed over, the comparison must
stop at that fold and name that field — which proves, without a GPU, that it
looks at everything it claims to.
"""
import os
import re
import subprocess

import pytest

from conftest import CSRC, GOLDEN, ORACLE_SO
import fold_cases as fc

TWIN = os.path.join(CSRC, "abpoa_amd_foldroundtwin")


@pytest.fixture(scope="module")
def twin(cputest_bin):
    if not os.path.exists(TWIN):
        subprocess.run(["make", "-j4", "cputest"], cwd=CSRC, check=True, stdout=subprocess.DEVNULL)
    return TWIN


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("foldround")
    ties = dict((os.path.basename(p)[:-3], p) for p in fc.tie_sets(d))
    return {"prefix": fc.prefix_staircase(d), "suffix": fc.suffix_staircase(d),
            "bubble": fc.bubble(d), "chains": fc.chain_sets(d), "ties": ties}


def _run(twin, args):
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    return subprocess.run([twin] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _clean(twin, args):
    p = _run(twin, args)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()[-500:]
    lines = p.stdout.splitlines()
    assert lines[-1].startswith(b"fold-round twin OK"), p.stdout
    return fc.parse_fold_check(lines[-2] + b"\n")


@pytest.mark.parametrize("rid", [[], ["-r1"]], ids=["norid", "rid"])
def test_unchanged_copy_passes_on_the_staircases(twin, inputs, rid):
    """Also pins what the GPU cases rely on: the staircases do drive one
    node's degree past the 64-entry sort array."""
    s = _clean(twin, rid + [inputs["prefix"]])
    assert s["folds"] == 76 and s["max_out_deg"] > 64, s
    s = _clean(twin, rid + [inputs["suffix"]])
    assert s["folds"] == 116 and s["max_in_deg"] > 64, s


def test_unchanged_copy_passes_on_row_count_edges(twin, inputs):
    for path, rows in zip(inputs["chains"], fc.CHAIN_ROWS):
        s = _clean(twin, [path])
        assert s["folds"] == 2 and s["rows_by_set"] == [rows] and s["min_n_rows"] == rows, s
    for path in inputs["ties"].values():
        s = _clean(twin, ["-r1", path])
        assert s["folds"] == fc.n_reads(path)


def test_unchanged_copy_passes_on_bubble_and_13_percent(twin, inputs):
    s = _clean(twin, [inputs["bubble"]])
    assert s["folds"] == 8 and s["max_n_rows"] == 452
    s = _clean(twin, ["-r1", os.path.join(GOLDEN, "synth13_seed1.fa")])
    assert s["folds"] == 24


# mutation -> the field the mismatch line must name
MUTATIONS = {
    "out_order": rb"out_(head|next)",   # whichever link of the chain comes first
    "out_tail": rb"out_tail",
    "rem": rb"rem",
    "n_span_read": rb"n_span_read",
    "pre_off": rb"pre_off",
    "pre_idx": rb"pre_idx",
    "row_remain": rb"row_remain",
    "n_out": rb"n_out",
}


@pytest.mark.parametrize("read", [1, 3])
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutation_is_caught(twin, inputs, mutation, read):
    """tie_l63_d4: two haplotypes alternating, so from read 1 on SRC and every
    variant site carry two out-edges of equal weight. One change at one read:
    exit 1, exactly one mismatch line, that set, read and field."""
    p = _run(twin, ["--mutate", "%s@%d" % (mutation, read), inputs["ties"]["tie_l63_d4"]])
    assert p.returncode == 1, p.stdout.decode() + p.stderr.decode()[-500:]
    bad = [ln for ln in p.stdout.splitlines() if ln.startswith(b"fold-check MISMATCH")]
    assert len(bad) == 1, p.stdout
    m = re.match(rb"fold-check MISMATCH set 0 read (\d+) field (\w+) index (-?\d+): device (-?\d+) twin (-?\d+)$",
                 bad[0])
    assert m, bad[0]
    assert int(m.group(1)) == read
    assert re.fullmatch(MUTATIONS[mutation], m.group(2)), bad[0]
    assert m.group(4) != m.group(5)
    assert p.stdout.splitlines()[-1] == b"fold-round twin FAILED"


def test_mutation_that_finds_no_place_is_an_error(twin, inputs):
    """A --mutate that never fired must not look like a pass: a chain has no
    node with two out-edges, and no read 7."""
    p = _run(twin, ["--mutate", "out_order@1", inputs["chains"][2]])
    assert p.returncode == 2 and b"never applied" in p.stderr
    p = _run(twin, ["--mutate", "n_out@7", inputs["chains"][2]])
    assert p.returncode == 2 and b"never applied" in p.stderr


def test_cpu_harness_refuses_fold_check(inputs, cputest_bin):
    """abpoa_amd_batchtest has no fold kernel: --fold-check there must fail
    rather than report a pass with nothing compared."""
    batchtest = os.path.join(CSRC, "abpoa_amd_batchtest")
    env = dict(os.environ)
    env["ABPOA_AMD_TEST_ALIGNER_SO"] = ORACLE_SO
    p = subprocess.run([batchtest, "--fold-check", inputs["chains"][0]], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 3, p.stderr.decode()[-500:]
    assert fc.parse_fold_check(p.stderr)["folds"] == 0
