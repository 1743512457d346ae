"""The device-resident batch driver on every workload and recovery path (-m gpu).

abpoa_amd_msa_batch -> gpu_batch_resident.cpp is the product's flagship path.
Its DP kernels read a CSR that the fold kernel built on the device, and width,
inf_min, use_remain, planes and the kernel pick are decided in build_jobs /
launch_slot, apart from the aligner seam's copy of those rules. Here
abpoa_amd_batchgpu (the batch harness linked with the GPU core) runs the driver
under the CLI's alignment options; the expected output of every set is the CPU
oracle's (abpoa_amd_cputest with liboracle.so injected, same options, -r2: all
read rows and the consensus row), never another run of the driver. The
harness's -S line carries the counters that prove which path a run took.
tests/test_batch_flags_cpu.py proves on the CPU that the harness parses like
the CLI; tests/test_arena_overflow_cpu.py that the overflow inputs overflow.

Every run is a child process: the knobs are read per call but the driver's
device allocations persist."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, CSRC, GPU_BIN
import batch_cases as bc

pytestmark = pytest.mark.gpu

BATCH_GPU = os.path.join(CSRC, "abpoa_amd_batchgpu")
KNOBS = ("ABPOA_AMD_MEM_GB", "ABPOA_AMD_GROUPS", "ABPOA_AMD_HOST_FOLD", "ABPOA_AMD_HOST_CONS",
         "ABPOA_AMD_HOST_MSA", "ABPOA_AMD_NODE_ALPHA", "ABPOA_AMD_SERIAL_FOLD",
         "ABPOA_AMD_DP_GENERIC", "ABPOA_AMD_DP_RING", "ABPOA_AMD_TEST_ALIGNER_SO")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resident")
    return {"ragged": bc.ragged(d), "amino": bc.amino(d), "mixed": bc.mixed(d),
            "overflow": bc.overflow_batch(d), "unaligned": [bc.unaligned_set(d)]}


def clean_env(extra=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(extra or {})
    return env


def resident(opts, files, env=None):
    """One batch call of the driver in a child: (records, counters)."""
    p = subprocess.run([BATCH_GPU] + list(opts) + ["-r2", "-S"] + files, env=clean_env(env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, "exit %d: %s" % (p.returncode, p.stderr.decode()[-2000:])
    return bc.records(p.stdout), bc.parse_stats(p.stderr)


PLANES = {"convex": 3, "affine": 3, "linear": 1}  # stored per cell (include/abpoa_amd.h)


def check(cputest_bin, oracle_env, opts, files, env=None, gap=None):
    """Run, compare every set with the oracle, and assert what every case
    asserts: one call, served by the resident driver, every set's consensus
    and rows from the device kernels, no fold redone serially. With `gap`
    also: the plane bytes are cells x planes of that gap model x the score
    width of the launches, when all launches had one width."""
    recs, st = resident(opts, files, env)
    print(st)
    bc.check_against_oracle(recs, cputest_bin, oracle_env, opts, files)
    assert (st["resident_calls"], st["hostfold_calls"]) == (1, 0), st
    assert st["cons_fallback_sets"] == 0 and st["msa_fallback_sets"] == 0 and st["fallback_folds"] == 0, st
    assert st["cons_device_sets"] == len(files) and st["cons_host_sets"] == 0, st
    assert st["msa_device_sets"] == len(files) and st["msa_host_sets"] == 0, st
    assert st["serial_folds"] == 0 and st["parallel_folds"] > 0, st
    assert st["launches_i16"] + st["launches_i32"] > 0, st
    assert st["noop_folds"] == 0, st  # no input gives an empty CIGAR
    assert st["dp_cells"] > 0, st
    if gap and (st["launches_i16"] == 0 or st["launches_i32"] == 0):
        width = 2 if st["launches_i32"] == 0 else 4
        assert st["alg_bytes"] == st["dp_cells"] * PLANES[gap] * width, st
    return st


# ---- (d) DP arena overflow: first in the file, it runs first -----------------
@pytest.mark.parametrize("gap", ["convex", "affine", "linear"])
def test_arena_overflow_retries(cputest_bin, oracle_env, inputs, gap):
    """D1 and D2 (batch_cases.overflow_set) with two ordinary sets. The four
    sets fall into three pipeline groups with D1 and D2 in different ones, so
    each overflowing job is a retry_failed call of its own. By the oracle's
    cell counts (test_arena_overflow_cpu.py) reads 2-4 of D1 need 1.5-1.6 x the
    reservation and reads 2-4 of D2 2.4-2.5 x: six jobs overflow, D1's succeed
    on their first retry launch and D2's overflow the doubled reservation once
    more (the `still` loop) and succeed at four times: 3 + 2 * 3 launches."""
    st = check(cputest_bin, oracle_env, bc.GAPS[gap], inputs["overflow"], gap=gap)
    assert st["dp_retry_jobs"] == 6, st
    assert st["dp_retry_launches"] == 9, st
    assert st["big_chunks"] == 0, st


def test_arena_overflow_sequential_cli(cputest_bin, oracle_env, inputs):
    """D1 through the sequential CLI: the aligner seam's retry slot
    (gpu_align.cpp), counted on the CLI's timing line."""
    fa = inputs["overflow"][0]
    p = subprocess.run([GPU_BIN, "-r2", fa], env=clean_env({"ABPOA_AMD_TIMING": "1"}),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rows = [ln for ln in p.stdout.decode().splitlines() if not ln.startswith(">")]
    assert rows == bc.oracle_rows(cputest_bin, oracle_env, [], fa)
    m = re.search(r"\[abamd timing cli\].* retry_jobs (\d+)", p.stderr.decode())
    assert m, p.stderr.decode()[-2000:]
    assert int(m.group(1)) == 3, m.group(0)  # reads 2-4, once each


# ---- (a) the workload matrix on the ragged batch -----------------------------
@pytest.mark.parametrize("wid,opts,keep", bc.WORKLOADS, ids=bc.WORKLOAD_IDS)
def test_workload_matrix(cputest_bin, oracle_env, inputs, wid, opts, keep):
    """Seven sets of depths 1-20 and 80-1500 bases under every gap model,
    alignment mode, band setting and score width bench.py can publish."""
    st = check(cputest_bin, oracle_env, opts, bc.workload_files(inputs["ragged"], keep),
               gap=wid.split("-")[0])
    if wid.endswith("-x45"):
        assert st["launches_i32"] > 0 and st["launches_i16"] == 0, st
    else:
        # int32 as well where graphs outgrow int16 (z-dropped reads fold their
        # unaligned tails in as new nodes)
        assert st["launches_i16"] > 0, st
    assert st["dp_retry_jobs"] == 0 and st["big_chunks"] == 0, st


# ---- (b) amino acids ---------------------------------------------------------
def test_amino_acids(cputest_bin, oracle_env, inputs):
    """m = 27 with BLOSUM62, affine as bench.py's aa workload. The aligned-pair
    pool of the capacity plan depends on m; whether it expands or not, the
    output is the oracle's."""
    st = check(cputest_bin, oracle_env, bc.AA_OPTS, inputs["amino"])
    assert st["launches_i16"] > 0 and st["launches_i32"] == 0, st


# ---- (c) mixed widths in one launch --------------------------------------------
def test_mixed_width_launch(cputest_bin, oracle_env, inputs):
    """300, 700 and 1300 bases at -M 30: the 1300 set picks int32 from its
    first alignment, so every launch that holds it runs at int32 and the other
    jobs of that launch get inf_min recomputed (build_jobs); the three sets are
    one group each, so the launches of the 300 set stay at int16."""
    st = check(cputest_bin, oracle_env, bc.MIXED_OPTS, inputs["mixed"], {"ABPOA_AMD_GROUPS": "1"})
    assert st["launches_i32"] == 7 and st["launches_i16"] == 0, st
    st = check(cputest_bin, oracle_env, bc.MIXED_OPTS, inputs["mixed"])
    assert st["launches_i32"] > 0 and st["launches_i16"] > 0, st
    st = check(cputest_bin, oracle_env, bc.MIXED_OPTS, inputs["mixed"][:1])
    assert st["launches_i16"] == 7 and st["launches_i32"] == 0, st


def test_int16_pick_in_int32_launch(cputest_bin, oracle_env, inputs):
    """The 32-bit inf_min recompute of build_jobs, where it decides the result.
    At the x45 scoring a 300-base job picks int16, where its score floor would
    be +14437 (alone it is refused). In one launch with a
    700-base job (ABPOA_AMD_GROUPS=1) it runs at int32 with the floor
    recomputed; with the int16 floor kept it would be positive at int32 and
    beat every real score. The oracle refuses that set alone too, so its
    expected output is the oracle's at the default scoring: x45 multiplies
    every score by 45, bands follow positions and not values, so as long as
    nothing overflows the alignments are the same
    (test_batch_flags_cpu.py::test_x45_scoring_is_scale_invariant shows it on
    the 700-base set, which the oracle serves at both)."""
    short, longer = inputs["ragged"][2], inputs["ragged"][3]
    x45 = bc.sc.GAPS_X45["convex"]
    recs, st = resident(x45, [short, longer], {"ABPOA_AMD_GROUPS": "1"})
    print(st)
    assert (st["resident_calls"], st["hostfold_calls"]) == (1, 0), st
    assert st["launches_i32"] == 6 and st["launches_i16"] == 0, st
    assert st["cons_fallback_sets"] == 0 and st["msa_fallback_sets"] == 0 and st["fallback_folds"] == 0, st
    for (cons, rows), want in ((recs[0], bc.oracle_rows(cputest_bin, oracle_env, [], short)),
                               (recs[1], bc.oracle_rows(cputest_bin, oracle_env, x45, longer))):
        assert rows == want and cons == want[-1].replace("-", "")


# ---- (e) big items and group counts ------------------------------------------
BIG = {"ABPOA_AMD_MEM_GB": "0.0005"}


def test_big_items(cputest_bin, oracle_env, inputs):
    """A 0.5 MB budget: every item of two or more jobs runs in budget-bounded
    chunks on the two big slots, and device_msa finds slot 0 without an arena."""
    st = check(cputest_bin, oracle_env, [], inputs["ragged"], BIG)
    assert st["big_chunks"] >= 3, st
    assert st["dp_retry_jobs"] == 0, st


def test_big_items_with_overflow(cputest_bin, oracle_env, inputs):
    """The retry slot while the big slots are in flight. D1 shares its group
    with the 3 x 300 set, so rounds 1 and 2 of that group are big items."""
    st = check(cputest_bin, oracle_env, [], inputs["overflow"], BIG)
    assert st["big_chunks"] > 0 and st["dp_retry_jobs"] == 6 and st["dp_retry_launches"] == 9, st


@pytest.mark.parametrize("groups", ["1", "2", "4"])
def test_group_counts(cputest_bin, oracle_env, inputs, groups):
    """Pipeline shapes other than the default three (slot 3 exists only for
    four), with items whose set list is empty because the depths differ."""
    st = check(cputest_bin, oracle_env, [], inputs["ragged"], {"ABPOA_AMD_GROUPS": groups})
    assert st["launches_i16"] > 0, st


# ---- (f) a read that aligns nowhere --------------------------------------------
def test_unaligned_read(cputest_bin, oracle_env, inputs):
    """Local mode, a poly-A read against a C/G/T graph: the candidate for an
    empty CIGAR gives a whole-read insertion instead, the
    fold takes it, and the reads after it still align correctly."""
    check(cputest_bin, oracle_env, bc.UNALIGNED_OPTS, inputs["unaligned"])


# ---- (g) sets with no graph ----------------------------------------------------
NO_GRAPH = r"""
import sys
sys.path.insert(0, %r)
import os
import numpy as np
import abpoa_amd, bench
sets = bench.gen_sets(np.random.default_rng(19), 3, depth=6, qlen=300)
sets = [sets[0], [], sets[1], [sets[2][0]], sets[2]]
out = {}
for driver in ("resident", "hostfold"):
    os.environ.pop("ABPOA_AMD_HOST_FOLD", None)
    if driver == "hostfold":
        os.environ["ABPOA_AMD_HOST_FOLD"] = "1"
    abpoa_amd.reset_batch_stats()
    out[driver] = abpoa_amd.msa_batch_results(sets, n_threads=2, out_msa=True)
    st = abpoa_amd.get_batch_stats()
    want = (1, 0) if driver == "resident" else (0, 1)
    assert (st["resident_calls"], st["hostfold_calls"]) == want, (driver, st)
a, b = out["resident"], out["hostfold"]
assert len(a) == len(b) == 5
for i, (x, y) in enumerate(zip(a, b)):
    assert x.keys() == y.keys()
    for k in x:
        assert x[k] == y[k], "set %%d field %%s: resident %%r host-fold %%r" %% (i, k, x[k], y[k])
assert a[1]["n_seq"] == 0 and a[1]["msa_len"] == 0 and a[1]["cons"] == []
assert a[3]["n_seq"] == 1 and len(a[3]["cons"]) == 1 and len(a[3]["cons"][0]) == len(sets[3][0])
print("no-graph OK")
"""


def test_sets_with_no_graph():
    """An empty set and a one-read set among ordinary ones, through the Python
    wrapper: the resident driver's result equals the host-fold driver's field
    for field."""
    p = subprocess.run([sys.executable, "-c", NO_GRAPH % ROOT], env=clean_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and b"no-graph OK" in p.stdout, \
        "exit %d: %s" % (p.returncode, p.stderr.decode()[-2000:])
