"""The batch harness parses like the CLI (no GPU needed).

tests/test_resident_paths_gpu.py drives the device-resident driver through
abpoa_amd_batchgpu with the CLI's alignment options and takes its expected
output from the sequential CPU CLI with the oracle injected. That comparison
means something only if the harness gives each option the CLI's effect, so for
every option set used there this runs abpoa_amd_batchtest (same source, linked
with the stub: host-fold driver, oracle injected through the seam) and wants
its records equal to the CLI's, per set. Also: the -S line, and the batch
counters of the CPU test library."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT, CSRC
import batch_cases as bc

BATCH_BIN = os.path.join(CSRC, "abpoa_amd_batchtest")
CPU_LIB = os.path.join(CSRC, "libabpoa_amd_cputest.so")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("batchflags")
    return {"ragged": bc.ragged(d), "amino": bc.amino(d), "mixed": bc.mixed(d),
            "overflow": bc.overflow_batch(d), "unaligned": [bc.unaligned_set(d)]}


def harness(oracle_env, opts, files, extra_env=None):
    env = dict(oracle_env)
    env.update(extra_env or {})
    p = subprocess.run([BATCH_BIN] + list(opts) + ["-r2", "-S"] + files, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return bc.records(p.stdout), bc.parse_stats(p.stderr)


def check(cputest_bin, oracle_env, opts, files):
    recs, st = harness(oracle_env, opts, files)
    bc.check_against_oracle(recs, cputest_bin, oracle_env, opts, files)
    # the CPU build has the host-fold driver only, and none of the device paths
    assert (st["resident_calls"], st["hostfold_calls"]) == (0, 1), st
    assert all(v == 0 for k, v in st.items() if k != "hostfold_calls"), st


@pytest.mark.parametrize("wid,opts,keep", bc.WORKLOADS, ids=bc.WORKLOAD_IDS)
def test_workload_options_parse_like_cli(cputest_bin, oracle_env, inputs, wid, opts, keep):
    check(cputest_bin, oracle_env, opts, bc.workload_files(inputs["ragged"], keep))


def test_amino_options_parse_like_cli(cputest_bin, oracle_env, inputs):
    check(cputest_bin, oracle_env, bc.AA_OPTS, inputs["amino"])
    # -c and the matrix are not idle: nucleotide scoring gives other rows
    plain = bc.oracle_rows(cputest_bin, oracle_env, ["-c"], inputs["amino"][2])
    assert plain != bc.oracle_rows(cputest_bin, oracle_env, bc.AA_OPTS, inputs["amino"][2])


def test_mixed_width_options_parse_like_cli(cputest_bin, oracle_env, inputs):
    check(cputest_bin, oracle_env, bc.MIXED_OPTS, inputs["mixed"])


@pytest.mark.parametrize("gap", ["convex", "affine", "linear"])
def test_overflow_batch_parses_like_cli(cputest_bin, oracle_env, inputs, gap):
    check(cputest_bin, oracle_env, bc.GAPS[gap], inputs["overflow"])


def test_unaligned_read_parses_like_cli(cputest_bin, oracle_env, inputs):
    check(cputest_bin, oracle_env, bc.UNALIGNED_OPTS, inputs["unaligned"])


def test_zdrop_fires_on_the_ragged_batch(cputest_bin, oracle_env, inputs):
    """The -m2 -z 5 workload is not idle: on at least one set of the ragged
    batch the oracle's rows differ from those of -m2 alone, for every gap."""
    for gap in ("convex", "affine", "linear"):
        g = bc.GAPS[gap]
        assert any(bc.oracle_rows(cputest_bin, oracle_env, g + ["-m2", "-z", "5"], fa) !=
                   bc.oracle_rows(cputest_bin, oracle_env, g + ["-m2"], fa)
                   for fa in inputs["ragged"]), gap


def test_x45_scoring_is_scale_invariant(cputest_bin, oracle_env, inputs):
    """What test_resident_paths_gpu.py::test_int16_pick_in_int32_launch rests
    on: the x45 scoring is the default one times 45, and where the oracle
    serves both (int32 for x45 from 400 bases on) the rows are the same."""
    for fa in inputs["ragged"][3:5]:
        assert bc.oracle_rows(cputest_bin, oracle_env, bc.sc.GAPS_X45["convex"], fa) == \
            bc.oracle_rows(cputest_bin, oracle_env, [], fa)
    # and the 300-base set alone is refused at x45
    p = subprocess.run([cputest_bin] + bc.sc.GAPS_X45["convex"] + ["-r2", inputs["ragged"][2]],
                       env=oracle_env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"unsupported scoring" in p.stderr, p.stderr[-500:]


def test_end_bonus_and_band_fraction_reach_abpt(cputest_bin, oracle_env, inputs):
    """-e and -f take the CLI's spelling too (-f changes the band and so may
    change rows; -e is never read in global mode: both must still parse)."""
    files = inputs["ragged"][2:4]
    check(cputest_bin, oracle_env, ["-b", "2", "-f", "0.0", "-e", "5"], files)
    assert bc.oracle_rows(cputest_bin, oracle_env, ["-b", "2", "-f", "0.0", "-e", "5"], files[1]) != \
        bc.oracle_rows(cputest_bin, oracle_env, [], files[1])


def test_harness_refuses_unknown_option(oracle_env, inputs):
    p = subprocess.run([BATCH_BIN, "-m", "7", inputs["ragged"][0]], env=oracle_env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"Unknown alignment mode" in p.stderr


def test_groups_do_not_change_the_ragged_batch(cputest_bin, oracle_env, inputs):
    """Items whose set list is empty (depths differ) under every group count."""
    base = harness(oracle_env, [], inputs["ragged"])[0]
    for g in ("1", "2", "4"):
        assert harness(oracle_env, [], inputs["ragged"], {"ABPOA_AMD_GROUPS": g})[0] == base, g


def test_batch_stats_api_cpu_library(cputest_bin, monkeypatch):
    """The CPU test library exports the batch counters; abpoa_amd.get_batch_stats()
    works against it and reports zeros after a reset."""
    h = ctypes.CDLL(CPU_LIB)
    v = [ctypes.c_uint64(7) for _ in range(10)]
    h.abpoa_amd_reset_batch_stats()
    h.abpoa_amd_get_batch_stats(*[ctypes.byref(x) for x in v])
    assert [x.value for x in v] == [0] * 10
    h.abpoa_amd_get_batch_stats.argtypes = [ctypes.c_void_p] * 10
    h.abpoa_amd_get_batch_stats(*([None] * 10))

    sys.path.insert(0, ROOT)
    import abpoa_amd
    monkeypatch.setenv("ABPOA_AMD_LIB", CPU_LIB)
    monkeypatch.setattr(abpoa_amd, "_lib", None)
    abpoa_amd.reset_batch_stats()
    st = abpoa_amd.get_batch_stats()
    assert set(st) == {"resident_calls", "hostfold_calls", "dp_retry_jobs", "dp_retry_launches",
                       "pool_expands", "big_chunks", "noop_folds", "seam_retry_jobs",
                       "launches_i16", "launches_i32"}
    assert all(x == 0 for x in st.values())
