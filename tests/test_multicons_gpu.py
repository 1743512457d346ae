"""Device multi-consensus (-m gpu): with ABPOA_AMD_DEVICE_MULTICONS=1 the
resident batch driver computes a max_n_cons > 1 call's consensus stage on the
GPU (read rows, het scan, per-cluster consensus kernels; only the candidate
columns come down for the host clustering). Every field of the callback
payload must equal the default graph-download + host path, every eligible set
must take the device path with no fallback and fewer downloaded bytes, the
inputs must produce one, two and three clusters of the sizes listed in
multicons_cases, and ineligible calls must stay on the host."""
import os

import numpy as np
import pytest

import multicons_cases as mc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SWITCH = "ABPOA_AMD_DEVICE_MULTICONS"
ON = {SWITCH: "1"}


def _run(sets, env=None, **kw):
    """(results, consensus stats, multicons stats) of one batch call with `env`
    set for its duration and the switch off unless `env` sets it."""
    import abpoa_amd
    env = dict(env or {})
    saved = {k: os.environ.get(k) for k in list(env) + [SWITCH]}
    os.environ.pop(SWITCH, None)
    os.environ.update(env)
    try:
        abpoa_amd.reset_cons_stats()
        abpoa_amd.reset_msa_stats()
        abpoa_amd.reset_multicons_stats()
        res = abpoa_amd.msa_batch_results(sets, n_threads=2, **kw)
        return res, abpoa_amd.get_cons_stats(), abpoa_amd.get_multicons_stats()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k] == y[k], "%s: set %d field %s differs" % (what, i, k)


def _cases(d):
    """[(name, reads, cluster sizes)] of the -d`d` batch."""
    out = []
    if d == 2:
        out += mc.tie_cases()
    for (seed, n_hap, depth, dd), sizes in sorted(mc.HAP_CASES.items()):
        if dd == d:
            out.append(("hap_s%d_h%d_n%d" % (seed, n_hap, depth), mc.hap_set(seed, n_hap, depth), sizes))
    for name, (dd, sizes) in sorted(mc.GOLDEN_CASES.items()):
        if dd == d:
            out.append((name, mc.golden_set(name), sizes))
    return out


@pytest.fixture(scope="module")
def ab_runs():
    """{d: (cases, on-run, off-run)}, computed once for the module."""
    runs = {}
    for d in (2, 3):
        cases = _cases(d)
        sets = [c[1] for c in cases]
        runs[d] = (cases, _run(sets, env=ON, max_n_cons=d), _run(sets, max_n_cons=d))
    return runs


@pytest.mark.parametrize("d", [2, 3])
def test_device_matches_host(ab_runs, d):
    cases, (dev, sd, md), (host, sh, mh) = ab_runs[d]
    n = len(cases)
    # switch off: the parent's behaviour, new counters untouched
    assert sh["device_sets"] == 0 and sh["host_sets"] == n and sh["fallback_sets"] == 0, sh
    assert all(v == 0 for v in mh.values()), mh
    # switch on: every set on the device, none fell back
    assert sd["device_sets"] == n and sd["host_sets"] == 0 and sd["fallback_sets"] == 0, sd
    assert md["device_sets"] == n and md["host_sets"] == 0 and md["fallback_sets"] == 0, md
    assert md["kernel_ns"] > 0 and sd["kernel_ns"] > 0
    _assert_same(dev, host, "device vs host multi-consensus (-d%d)" % d)
    assert 0 < sd["d2h_bytes"] < sh["d2h_bytes"], (sd, sh)
    assert md["d2h_bytes"] == sd["d2h_bytes"]
    # the inputs did their job
    for (name, reads, sizes), r in zip(cases, dev):
        assert r["n_seq"] == len(reads)
        assert r["clu_n_seq"] == sizes, name
        assert len(r["cons"]) == len(sizes)
        for ids, size in zip(r["clu_read_ids"], sizes):
            assert len(ids) == size
        for ci in range(len(sizes)):
            assert len(r["cons"][ci]) == len(r["cov"][ci]) == len(r["phred"][ci]) == len(r["node_ids"][ci]) > 0
    assert md["one_cluster_sets"] == sum(1 for r in dev if len(r["cons"]) == 1)
    assert md["clusters"] == sum(len(r["cons"]) for r in dev)
    assert md["cand_cols"] > 0


def test_one_two_and_three_clusters_occur(ab_runs):
    seen = set()
    for d in (2, 3):
        seen |= {len(r["cons"]) for r in ab_runs[d][1][0]}
    assert seen == {1, 2, 3}


def _golden_text(res):
    lines = []
    for r in res:
        for ci, seq in enumerate(r["cons"]):
            lines.append(">Consensus_sequence_%d %s" % (ci + 1, ",".join(str(x) for x in r["clu_read_ids"][ci])))
            lines.append(seq)
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("name,d,expected", [("heter.fa", 2, "expected_heter_d2.txt"),
                                             ("3alleles.fa", 3, "expected_3alleles_d3.txt")])
def test_reference_anchor(name, d, expected):
    """The device path reproduces the committed reference output, read-id
    lists included."""
    res, st, m = _run([mc.golden_set(name)], env=ON, max_n_cons=d)
    assert st["device_sets"] == 1 and st["host_sets"] == 0 and m["device_sets"] == 1, (st, m)
    assert _golden_text(res) == open(os.path.join(GOLDEN, expected)).read()


def _msa_sets():
    return [mc.hap_set(1, 2), mc.hap_set(2, 1), mc.hap_set(1, 3), mc.golden_set("heter.fa"),
            mc.tie_cases()[0][1]]


@pytest.mark.parametrize("out_cons", [True, False])
def test_out_msa(out_cons):
    import abpoa_amd
    sets = _msa_sets()
    dev, sd, md = _run(sets, env=ON, max_n_cons=3, out_msa=True, out_cons=out_cons)
    msa_dev = abpoa_amd.get_msa_stats()
    assert sd["device_sets"] == len(sets) and sd["fallback_sets"] == 0, sd
    assert md["device_sets"] == len(sets) and md["fallback_sets"] == 0, md
    assert msa_dev["device_sets"] == len(sets) and msa_dev["host_sets"] == 0, msa_dev
    assert msa_dev["d2h_bytes"] > 0 and msa_dev["kernel_ns"] > 0
    host, sh, mh = _run(sets, max_n_cons=3, out_msa=True, out_cons=out_cons)
    assert sh["device_sets"] == 0 and all(v == 0 for v in mh.values())
    _assert_same(dev, host, "device vs host rows (out_cons=%s)" % out_cons)
    assert {len(r["cons"]) for r in dev} == {1, 2, 3}
    for r, s in zip(dev, sets):
        assert r["msa_len"] > 0
        assert len(r["msa"]) == len(s) + (len(r["cons"]) if out_cons else 0)
        assert all(len(row) == r["msa_len"] for row in r["msa"])


def test_pool_expansion():
    """Tiny ABPOA_AMD_NODE_ALPHA forces pool overflows mid-run: the stage must
    work on the re-carved (expanded) slab, whose regions it maps from node_cap."""
    import abpoa_amd
    sets = [mc.hap_set(1, 2), mc.hap_set(7, 3), mc.hap_set(2, 1)]
    abpoa_amd.reset_batch_stats()
    env = dict(ON)
    env["ABPOA_AMD_NODE_ALPHA"] = "0.02"
    tight, st, mt = _run(sets, env=env, max_n_cons=3, out_msa=True)
    assert abpoa_amd.get_batch_stats()["pool_expands"] > 0, "the knob forced no expansion"
    abpoa_amd.reset_batch_stats()
    assert st["device_sets"] == 3 and st["fallback_sets"] == 0 and mt["device_sets"] == 3, (st, mt)
    roomy, sr, mr = _run(sets, env=ON, max_n_cons=3, out_msa=True)
    assert abpoa_amd.get_batch_stats()["pool_expands"] == 0
    assert sr["device_sets"] == 3 and mr["device_sets"] == 3
    _assert_same(tight, roomy, "pool-expansion vs roomy")
    host, _sh, _mh = _run(sets, max_n_cons=3, out_msa=True)
    _assert_same(tight, host, "pool-expansion vs host")


def test_odd_batch():
    """A one-read set, a two-read set and a set with no reads among others."""
    full = mc.hap_set(1, 2)
    sets = [full[:1], full, full[:2], [], mc.tie_cases()[1][1]]
    dev, sd, md = _run(sets, env=ON, max_n_cons=2)
    host, sh, mh = _run(sets, max_n_cons=2)
    _assert_same(dev, host, "odd batch")
    # the empty set has no graph: it takes the host path on either setting
    assert sd["device_sets"] == 4 and sd["host_sets"] == 1 and sd["fallback_sets"] == 0, sd
    assert md["device_sets"] == 4 and md["host_sets"] == 1 and md["fallback_sets"] == 0, md
    assert [len(r["cons"]) for r in dev] == [1, 2, 1, 0, 2]
    assert md["one_cluster_sets"] == 2


@pytest.mark.parametrize("env,kw", [({}, {"cons_algrm": "MF"}), ({"ABPOA_AMD_HOST_CONS": "1"}, {})],
                         ids=["MF", "HOST_CONS"])
def test_ineligible_with_the_switch_on(env, kw):
    rng = np.random.default_rng(55)
    sets = [mc.hap_set(1, 2), mc.hap_set(7, 2), [rng.integers(0, 4, 80, dtype=np.uint8).tobytes()] * 3]
    e = dict(ON)
    e.update(env)
    res, st, m = _run(sets, env=e, max_n_cons=2, **kw)
    assert st["device_sets"] == 0 and st["host_sets"] == 3 and st["fallback_sets"] == 0, st
    assert m["device_sets"] == 0 and m["host_sets"] == 3 and m["kernel_ns"] == 0, m
    off, _so, mo = _run(sets, env=env, max_n_cons=2, **kw)
    assert all(v == 0 for v in mo.values())
    _assert_same(res, off, "ineligible call, switch on vs off")
