"""Device consensus (-m gpu): with the default configuration the resident
batch driver computes each set's consensus on the GPU (abamd_cons_kernel) and
downloads only the consensus. Every field of the callback payload must be
byte-identical to the graph-download + host consensus path
(ABPOA_AMD_HOST_CONS=1), every eligible set must take the device path with
zero fallbacks, and ineligible configurations must stay on the host path."""
import importlib
import os
import sys

import numpy as np
import pytest

import cons_cases
from conftest import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)


def _bench():
    return importlib.import_module("bench")


def _run(sets, env=None, **kw):
    """(results, stats) of one batch call with `env` set for its duration."""
    import abpoa_amd
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        abpoa_amd.reset_cons_stats()
        res = abpoa_amd.msa_batch_results(sets, n_threads=2, **kw)
        stats = abpoa_amd.get_cons_stats()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, stats


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k] == y[k], "%s: set %d field %s differs" % (what, i, k)


def _device_vs_host(sets):
    os.environ.pop("ABPOA_AMD_HOST_CONS", None)
    dev, st = _run(sets)
    assert st["device_sets"] == len(sets), st
    assert st["fallback_sets"] == 0 and st["host_sets"] == 0, st
    assert st["d2h_bytes"] > 0
    host, sh = _run(sets, env={"ABPOA_AMD_HOST_CONS": "1"})
    assert sh["device_sets"] == 0 and sh["host_sets"] == len(sets), sh
    assert sh["fallback_sets"] == 0 and sh["kernel_ns"] == 0, sh
    _assert_same(dev, host, "device vs host consensus")
    return dev, st, sh


def test_device_path_matches_host_path():
    rng = np.random.default_rng(321)
    sets = _bench().gen_sets(rng, 6, depth=15, qlen=600)
    sets[1] = sets[1][:1]   # a single read: pure chain graph
    sets[4] = sets[4][:2]
    dev, st, sh = _device_vs_host(sets)
    for r, s in zip(dev, sets):
        assert r["n_seq"] == len(s) and len(r["cons"]) == 1
        assert r["clu_n_seq"] == [len(s)] and r["clu_read_ids"] == [list(range(len(s)))]
        assert len(r["cons"][0]) == len(r["cov"][0]) == len(r["phred"][0]) == len(r["node_ids"][0])
    # only the consensus comes back: far fewer bytes than the graph download
    assert st["d2h_bytes"] < sh["d2h_bytes"]


def test_tie_stress_and_boundary_lengths():
    sets = [reads for _name, reads in cons_cases.all_sets()]
    _device_vs_host(sets)


def test_reference_anchor():
    """seq.fa on the device path reproduces the committed reference output."""
    reads, cur = [], None
    for line in open(os.path.join(GOLDEN, "seq.fa")):
        line = line.strip()
        if line.startswith(">"):
            cur = []
            reads.append(cur)
        elif line:
            cur.append(line)
    sets = [[bytes("ACGT".index(c) for c in "".join(parts).upper()) for parts in reads]]
    res, st = _run(sets)
    assert st["device_sets"] == 1 and st["host_sets"] == 0, st
    expected = "".join(open(os.path.join(GOLDEN, "expected_seq_cons.txt")).read().splitlines()[1:])
    assert res[0]["cons"] == [expected]


def test_pool_expansion_device_path():
    """Tiny ABPOA_AMD_NODE_ALPHA forces pool overflows mid-run: the consensus
    kernel must work on the re-carved (expanded) slab."""
    rng = np.random.default_rng(77)
    sets = _bench().gen_sets(rng, 3, depth=20, qlen=500)
    import abpoa_amd
    abpoa_amd.reset_batch_stats()
    tight, st = _run(sets, env={"ABPOA_AMD_NODE_ALPHA": "0.02"})
    assert abpoa_amd.get_batch_stats()["pool_expands"] > 0, "the knob forced no expansion"
    abpoa_amd.reset_batch_stats()
    assert st["device_sets"] == 3 and st["fallback_sets"] == 0 and st["host_sets"] == 0, st
    roomy, sr = _run(sets)
    assert sr["device_sets"] == 3 and sr["host_sets"] == 0, sr
    assert abpoa_amd.get_batch_stats()["pool_expands"] == 0
    _assert_same(tight, roomy, "pool-expansion vs roomy")


@pytest.mark.parametrize("kw", [{"cons_algrm": "MF"}, {"max_n_cons": 2}],
                         ids=["MF", "max_n_cons2"])
def test_ineligible_configurations_stay_on_host(kw):
    rng = np.random.default_rng(55)
    sets = _bench().gen_sets(rng, 3, depth=12, qlen=400)
    res, st = _run(sets, **kw)
    assert st["device_sets"] == 0 and st["host_sets"] == 3 and st["fallback_sets"] == 0, st
    hostfold, _ = _run(sets, env={"ABPOA_AMD_HOST_FOLD": "1"}, **kw)
    _assert_same(res, hostfold, "resident vs host-fold (%s)" % kw)
