"""Device row-column MSA (-m gpu): with abpt->out_msa and the default
configuration the resident batch driver builds each set's alignment matrix on
the GPU (abamd_msa_rank_kernel + abamd_msa_place_kernel) and downloads only the
matrix. Every field of the callback payload, rows included, must be
byte-identical to the graph-download + abpoa_generate_rc_msa path
(ABPOA_AMD_HOST_MSA=1); every eligible set must take the device path with zero
fallbacks; ineligible configurations must stay on the host path; and without
out_msa nothing changes."""
import importlib
import os
import sys

import numpy as np
import pytest

import cons_cases
from conftest import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)

ZERO = {"device_sets": 0, "host_sets": 0, "fallback_sets": 0, "d2h_bytes": 0, "kernel_ns": 0}


def _bench():
    return importlib.import_module("bench")


def _run(sets, env=None, **kw):
    """(results, msa stats, cons stats) of one batch call with `env` set for
    its duration."""
    import abpoa_amd
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        abpoa_amd.reset_cons_stats()
        abpoa_amd.reset_msa_stats()
        res = abpoa_amd.msa_batch_results(sets, n_threads=2, **kw)
        stats = abpoa_amd.get_msa_stats()
        cstats = abpoa_amd.get_cons_stats()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, stats, cstats


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k] == y[k], "%s: set %d field %s differs" % (what, i, k)


def _decode(read):
    return "".join("ACGT"[c] for c in read)


def _check_structure(res, sets, out_cons):
    """Properties every row-column MSA has, checked on the device result."""
    for r, s in zip(res, sets):
        rows, ln = r["msa"], r["msa_len"]
        assert len(rows) == len(s) + (1 if out_cons else 0)
        assert ln > 0 and all(len(row) == ln for row in rows)
        assert set("".join(rows)) <= set("ACGTN-")
        for row, read in zip(rows, s):
            assert row.replace("-", "") == _decode(read)
        if out_cons:
            assert rows[-1].replace("-", "") == r["cons"][0]
        # no all-gap column among the read rows
        mat = np.frombuffer("".join(rows[:len(s)]).encode(), dtype=np.uint8).reshape(len(s), ln)
        assert not (mat == ord("-")).all(axis=0).any()


def _device_vs_host(sets, out_cons):
    for k in ("ABPOA_AMD_HOST_MSA", "ABPOA_AMD_HOST_CONS"):
        os.environ.pop(k, None)
    dev, st, cst = _run(sets, out_msa=True, out_cons=out_cons)
    assert st["device_sets"] == len(sets), st
    assert st["fallback_sets"] == 0 and st["host_sets"] == 0, st
    assert st["d2h_bytes"] > 0 and st["kernel_ns"] > 0, st
    assert cst["device_sets"] == len(sets) and cst["host_sets"] == 0, cst
    host, sh, csh = _run(sets, env={"ABPOA_AMD_HOST_MSA": "1"}, out_msa=True, out_cons=out_cons)
    assert sh["device_sets"] == 0 and sh["host_sets"] == len(sets), sh
    assert sh["fallback_sets"] == 0 and sh["kernel_ns"] == 0, sh
    # a set is device for both stages or host for both
    assert csh["device_sets"] == 0 and csh["host_sets"] == len(sets), csh
    _assert_same(dev, host, "device vs host MSA (out_cons=%s)" % out_cons)
    _check_structure(dev, sets, out_cons)
    return dev, st, sh


@pytest.mark.parametrize("out_cons", [True, False], ids=["cons_row", "reads_only"])
def test_device_path_matches_host_path(out_cons):
    rng = np.random.default_rng(321)
    sets = _bench().gen_sets(rng, 6, depth=15, qlen=600)
    sets[1] = sets[1][:1]   # a single read: pure chain graph, no gaps
    sets[4] = sets[4][:2]
    dev, st, sh = _device_vs_host(sets, out_cons)
    # Byte budget at depth 15: the graph download is >= 65 B per node (33 B of
    # node arrays, >= 32 B per edge, at least one edge per node); the matrix is
    # n_seq + 1 B per column with columns <= nodes. Not asserted above depth 50.
    assert st["d2h_bytes"] < sh["d2h_bytes"], (st, sh)


@pytest.mark.parametrize("out_cons", [True, False], ids=["cons_row", "reads_only"])
def test_tie_stress_and_boundary_lengths(out_cons):
    sets = [reads for _name, reads in cons_cases.all_sets()]
    _device_vs_host(sets, out_cons)


@pytest.mark.parametrize("out_cons", [True, False], ids=["cons_row", "reads_only"])
def test_bitset_word_boundary(out_cons):
    """Depth 64 is the last set with one read-id word per edge, 65 the first
    with two."""
    rng = np.random.default_rng(99)
    sets = [_bench().gen_sets(rng, 1, depth=d, qlen=300)[0] for d in (64, 65, 80)]
    _device_vs_host(sets, out_cons)


def _seq_fa_sets():
    reads, cur = [], None
    for line in open(os.path.join(GOLDEN, "seq.fa")):
        line = line.strip()
        if line.startswith(">"):
            cur = []
            reads.append(cur)
        elif line:
            cur.append(line)
    return [[bytes("ACGT".index(c) for c in "".join(parts).upper()) for parts in reads]]


@pytest.mark.parametrize("out_cons,golden", [(True, "expected_seq_r2.txt"),
                                             (False, "expected_seq_r1.txt")],
                         ids=["r2", "r1"])
def test_reference_anchor(out_cons, golden):
    """seq.fa on the device path reproduces the committed reference rows."""
    res, st, _ = _run(_seq_fa_sets(), out_msa=True, out_cons=out_cons)
    assert st["device_sets"] == 1 and st["host_sets"] == 0 and st["fallback_sets"] == 0, st
    expected = [ln for ln in open(os.path.join(GOLDEN, golden)).read().splitlines()
                if not ln.startswith(">")]
    assert res[0]["msa"] == expected
    assert res[0]["msa_len"] == len(expected[0])


def test_pool_expansion_device_path():
    """Tiny ABPOA_AMD_NODE_ALPHA forces pool overflows mid-run: the MSA
    kernels' workspaces must hold on the re-carved (expanded) slab."""
    rng = np.random.default_rng(77)
    sets = _bench().gen_sets(rng, 3, depth=20, qlen=500)
    import abpoa_amd
    abpoa_amd.reset_batch_stats()
    tight, st, _ = _run(sets, env={"ABPOA_AMD_NODE_ALPHA": "0.02"}, out_msa=True)
    assert abpoa_amd.get_batch_stats()["pool_expands"] > 0, "the knob forced no expansion"
    abpoa_amd.reset_batch_stats()
    assert st["device_sets"] == 3 and st["fallback_sets"] == 0 and st["host_sets"] == 0, st
    roomy, sr, _ = _run(sets, out_msa=True)
    assert sr["device_sets"] == 3 and sr["host_sets"] == 0, sr
    assert abpoa_amd.get_batch_stats()["pool_expands"] == 0
    _assert_same(tight, roomy, "pool-expansion vs roomy")
    _check_structure(tight, sets, True)


@pytest.mark.parametrize("kw", [{"cons_algrm": "MF"}, {"max_n_cons": 2}],
                         ids=["MF", "max_n_cons2"])
def test_host_only_configurations(kw):
    rng = np.random.default_rng(55)
    sets = _bench().gen_sets(rng, 3, depth=12, qlen=400)
    res, st, _ = _run(sets, out_msa=True, **kw)
    assert st["device_sets"] == 0 and st["host_sets"] == 3 and st["fallback_sets"] == 0, st
    assert st["kernel_ns"] == 0, st
    hostfold, _, _ = _run(sets, env={"ABPOA_AMD_HOST_FOLD": "1"}, out_msa=True, **kw)
    _assert_same(res, hostfold, "resident vs host-fold (%s)" % kw)
    for r, s in zip(res, sets):
        assert len(r["msa"]) == len(s) + len(r["cons"])
        for row, read in zip(r["msa"], s):
            assert row.replace("-", "") == _decode(read)
        for row, cons in zip(r["msa"][len(s):], r["cons"]):
            assert row.replace("-", "") == cons


def test_no_side_effects_without_out_msa():
    rng = np.random.default_rng(11)
    sets = _bench().gen_sets(rng, 3, depth=8, qlen=300)
    res, st, cst = _run(sets, env={"ABPOA_AMD_HOST_MSA": "1"})
    assert st == ZERO
    # ABPOA_AMD_HOST_MSA matters only with out_msa: still the device consensus
    assert cst["device_sets"] == 3 and cst["host_sets"] == 0, cst
    for r in res:
        assert "msa" not in r and "msa_len" not in r
        assert sorted(r) == sorted(["n_seq", "cons", "node_ids", "cov", "phred",
                                    "clu_n_seq", "clu_read_ids"])
