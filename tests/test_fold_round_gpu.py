"""The production fold kernel's own outputs, after every fold (-m gpu).

abamd_fold_round_kernel (gpu_fold.hip) is the only fold code a batch job runs,
and its topo BFS, adjacency sort (both branches), remain chunks, n_span and
CSR prefix scan exist nowhere else; the validation kernels abpoa_amd_foldgpu
drives end in the serial bodies instead. Final consensus and MSA text is a weak
witness for them: an off-by-one max_remain only moves a band edge, the order of
equal-weight edges only picks among ties, and no committed input had a node of
degree above 64.

Here abpoa_amd_batchgpu --fold-check installs the resident driver's fold probe
and compares, after EVERY fold of every set, what the kernel left in the set's
slab with a host twin advanced by the serial abamd_flat_* passes
(abamd_fold_round_check.c): counters, every pool and chain array with heads
and tails, read-id bitsets, the topological order and its inverse up to SINK,
max_remain, and the seven DP-row CSR arrays — in the production workspace
aliasing and slab layout, pool growth and retry launches included. The twin is
pinned to the pointer graph on the same inputs by tests/test_fold_twin.py, the
comparison itself by tests/test_fold_round_twin.py.

Every run is a child process; each case asserts exit status 0, one compared
fold per read, no walk redone serially, and the path fact it exists for, read
from the harness's [fold-check] line or its [batch-stats] line."""
import os
import subprocess

import pytest

from conftest import CSRC, GOLDEN
import batch_cases as bc
import fold_cases as fc
import seam_cases as sc

pytestmark = pytest.mark.gpu

BATCH_GPU = os.path.join(CSRC, "abpoa_amd_batchgpu")
KNOBS = ("ABPOA_AMD_MEM_GB", "ABPOA_AMD_GROUPS", "ABPOA_AMD_HOST_FOLD", "ABPOA_AMD_HOST_CONS",
         "ABPOA_AMD_HOST_MSA", "ABPOA_AMD_NODE_ALPHA", "ABPOA_AMD_SERIAL_FOLD",
         "ABPOA_AMD_DP_GENERIC", "ABPOA_AMD_DP_RING", "ABPOA_AMD_TEST_ALIGNER_SO")
RID = ["-r2"]  # rows requested: read ids tracked, rid_pool compared


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("foldround")
    return {"prefix": [fc.prefix_staircase(d)], "suffix": [fc.suffix_staircase(d)],
            "chains": fc.chain_sets(d), "ties": fc.tie_sets(d), "bubble": [fc.bubble(d)],
            "golden": [os.path.join(GOLDEN, "3alleles.fa"), os.path.join(GOLDEN, "heter.fa")],
            "synth13": [sc.SYNTH13_SEED1], "amino": [fc.amino(d)],
            "ragged": bc.ragged(d), "low_alpha": [fc.low_alpha(d)],
            "D1": [bc.overflow_set(d, "D1")]}


def fold_check(opts, files, env=None, serial=False):
    """One batch call under --fold-check: ([fold-check] line, [batch-stats] line)."""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    p = subprocess.run([BATCH_GPU, "--fold-check", "-S"] + list(opts) + files, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, "exit %d: %s" % (p.returncode, p.stderr.decode()[-2000:])
    s, st = fc.parse_fold_check(p.stderr), bc.parse_stats(p.stderr)
    print(s, st)
    reads = sum(fc.n_reads(f) for f in files)
    assert s["folds"] == reads and s["noop"] == 0, s
    assert s["fallback"] == 0 and st["fallback_folds"] == 0, (s, st)
    assert (st["resident_calls"], st["hostfold_calls"]) == (1, 0), st
    if serial:
        assert (s["serial"], s["parallel"]) == (reads, 0), s
    else:
        assert (s["serial"], s["parallel"]) == (0, reads), s
    assert (st["serial_folds"], st["parallel_folds"]) == (s["serial"], s["parallel"]), (s, st)
    return s, st


# ---- the sort branches ------------------------------------------------------
def test_prefix_staircase_out_degree_past_64(inputs):
    """SRC's out-chain grows by one edge per read, through 64 (private array)
    and 65 (in-place chain selection), and the repeats make later edges
    heavier, so both branches reorder. Two read-id words."""
    s, _ = fold_check(RID, inputs["prefix"])
    assert s["max_out_deg"] > 64, s


def test_suffix_staircase_in_degree_past_64(inputs):
    s, _ = fold_check(RID, inputs["suffix"])
    assert s["max_in_deg"] > 64, s


# ---- row-count edges: the CSR prefix scan's rows per lane, the remain chunks --
def test_chain_row_counts(inputs):
    s, _ = fold_check(RID, inputs["chains"])
    assert tuple(s["rows_by_set"]) == fc.CHAIN_ROWS == (3, 63, 64, 65, 127, 128, 129), s
    assert (s["min_n_rows"], s["max_n_rows"]) == (3, 129), s


def test_tie_stress_sets(inputs):
    """Equal-weight edge pairs at SRC and at every variant site: their order
    is the sort's stability, which final text sees only through tie rules."""
    s, _ = fold_check(RID, inputs["ties"])
    assert s["max_out_deg"] >= 2 and s["max_in_deg"] >= 2, s


# ---- far successors next to in-chunk ones -----------------------------------
def test_bubble_far_successors(inputs):
    s, _ = fold_check(RID, inputs["bubble"])
    assert s["max_n_rows"] == 452, s   # 300 + 150 + SRC + SINK: the bubble is in the graph


# ---- aligned groups and wide rows --------------------------------------------
def test_golden_allele_sets(inputs):
    fold_check(RID, inputs["golden"])


@pytest.mark.parametrize("opts", [[], RID], ids=["norid", "rid"])
def test_13_percent(inputs, opts):
    """Without -r2 no read ids are tracked (rid_n = 0): the benchmark's layout."""
    s, _ = fold_check(opts, inputs["synth13"])
    assert s["max_in_deg"] >= 5, s


def test_amino_blosum(inputs):
    """m = 27: aligned groups up to 26 wide, and the aligned-pool pre-check."""
    fold_check(fc.AA_OPTS + RID, inputs["amino"])


# ---- modes that change what the fold sees -------------------------------------
@pytest.mark.parametrize("mode", ["-m1", "-m2"])
def test_local_and_extend_cigars(inputs, mode):
    """CIGARs with end insertions and clipped ends."""
    fold_check([mode] + RID, inputs["synth13"])


def test_unbanded_no_remain(inputs):
    """-b -1 and no z-drop: use_remain = 0, row_remain must be all zero and
    the remain pass is skipped."""
    fold_check(["-b", "-1"] + RID, inputs["synth13"])


def test_serial_walk(inputs):
    fold_check(RID, inputs["synth13"], env={"ABPOA_AMD_SERIAL_FOLD": "1"}, serial=True)


# ---- driver paths --------------------------------------------------------------
@pytest.mark.parametrize("groups", ["1", "3"])
def test_ragged_several_jobs_per_launch(inputs, groups):
    fold_check(RID, inputs["ragged"], env={"ABPOA_AMD_GROUPS": groups})


def test_pool_growth_relaunches(inputs):
    """ABPOA_AMD_NODE_ALPHA=0.02 plans pools far too small for 20 x 500 at
    10 % error: folds hit the pre-check, expand_set copies only the pools, and
    the relaunched fold must rewrite every derived array in the new slab."""
    s, st = fold_check(RID, inputs["low_alpha"], env={"ABPOA_AMD_NODE_ALPHA": "0.02"})
    assert s["caps_grew"] == 1, s
    assert st["pool_expands"] > 0, st


def test_retry_slot_carries_the_fold(inputs):
    """D1: the DP arena overflows, the fold is skipped, and the retry launch's
    own fold pass catches the graph up."""
    s, st = fold_check(RID, inputs["D1"])
    assert st["dp_retry_jobs"] > 0, st
