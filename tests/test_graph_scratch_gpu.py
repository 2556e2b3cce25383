"""The three graph calls of a context (selhip_ctx_spanning_forest, selhip_ctx_cluster_greedy, selhip_ctx_cluster) share one set of
scratch buffers (GraphScratch): this test runs them one behind the other on ONE context while the database is
replaced by a larger and then by the first set again, so that a call meets buffers another call sized and filled -- too small before
they regrow, then larger than needed and full of the other set's values.  Every output is compared with the host models
(tests/forest_model.py, greedy_model.py, cluster_model.py) on the records fetched from the pass, byte for byte where the tests of each
call compare bytes; the free-standing entries, whose scratch is one carved block per call, run between the legs on the same pairs."""
import numpy as np
import pytest

import cluster_model as CM
import forest_model as FM
import greedy_model as GM
import smhc_model as M
from test_cluster_gpu import assert_same as same_clusters, raw_cluster
from test_forest_gpu import raw_forest
from test_greedy_gpu import assert_same as same_greedy, raw_greedy

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_SMH_A, MODE_CB_SMH, Selector

pytestmark = pytest.mark.gpu

M_BUCKETS = 256
ORDER = ("forest", "greedy", "cluster", "greedy", "forest", "cluster")
SMALL, LARGE = 70, 300          # more than one wave and less than one 256-thread block; more than one block: every buffer regrows


@pytest.fixture
def grid_hook():
    """sets the process-wide grid of the record kernels (0 = automatic) and puts the default back"""
    with Selector(0) as sel:
        def set_hooks(blocks, vertex_blocks=0):
            sel.set_param("cluster_blocks", blocks)
            sel.set_param("vertex_blocks", vertex_blocks)
            assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (blocks, vertex_blocks)
        yield set_hooks
        set_hooks(0, 0)


def load(sel, oracle, n):
    """the planted-group set of n genomes uploaded, one all-pairs pass run: (records, the two cuts, the models' answers per cut)"""
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, M_BUCKETS, 77 + n))
    sel.upload(hll, aux, cards)
    sel.set_criterion(CRIT_SMH_A)
    rec = sel.run(0.3, MODE_CB_SMH, 2, 128)
    values = np.unique(rec["jaccard"])
    assert len(values) > 1
    cuts = (-np.inf, float(values[len(values) // 2]))
    recs = FM.records_of_pass(rec)
    want = {}
    for cut in cuts:
        k, lab = FM.kruskal(recs, n, cut)
        want[cut] = {"forest": (FM.as_records(k).tobytes(), lab, FM.boruvka_rounds(recs, n, cut)[2]),
                     "greedy": GM.clusters(rec, n, cut, "max_degree"),
                     "cluster": CM.clusters(CM.record_edges(rec, cut), n, "max_degree")}
        assert 1 < want[cut]["cluster"]["n_clusters"] < n and 0 < len(k) < n - 1          # a non-trivial list
    return rec, cuts, want


def leg(sel, cuts, want, what):
    """the six calls at both cuts, each against its model; returns every output's bytes, in call order"""
    n, out = sel.n, []
    for cut in cuts:
        for kind in ORDER:
            if kind == "forest":
                got = raw_forest(sel, cut)
                edges, lab, rounds = want[cut]["forest"]
                assert got["edges"].tobytes() == edges and got["labels"].tolist() == lab and got["rounds"] == rounds, (what, cut, kind)
                assert got["n_edges"] == n - want[cut]["cluster"]["n_clusters"], (what, cut)
                out.append((got["edges"].tobytes(), got["labels"].tobytes(), got["rounds"]))
            elif kind == "greedy":
                got = raw_greedy(sel, cut, 0)
                same_greedy(got, want[cut]["greedy"], (what, cut, kind))
                out.append(tuple(sorted((k, v.tobytes()) for k, v in got.items() if k not in ("rounds", "n_clusters"))) + (got["n_clusters"],))
            else:
                got = raw_cluster(sel, cut, 0)
                same_clusters(got, want[cut]["cluster"], (what, cut, kind))
                out.append(tuple(sorted((k, v.tobytes()) for k, v in got.items() if k != "n_clusters")) + (got["n_clusters"],))
    return out


def free_standing(sel, rec, what):
    """selhip_components, selhip_greedy_representatives and selhip_spanning_forest on the pass's pairs, beside the context's calls"""
    n = sel.n
    pairs = np.stack([rec["i"], rec["k"]], axis=1).astype(np.int32)
    labels = pkg.components(pairs, n)
    assert np.array_equal(labels, CM.labels(pairs, n)) and np.array_equal(labels, raw_cluster(sel, -np.inf, 0)["labels"]), what
    is_rep, rounds = pkg.greedy_representatives(pairs, n)                                 # key = vertex: the order of "max_rank"
    by_rank = raw_greedy(sel, -np.inf, 2)
    assert np.array_equal(is_rep.astype(bool), GM.representatives(pairs, n)), what
    assert np.array_equal(np.flatnonzero(is_rep), np.sort(by_rank["representatives"])) and rounds >= 1, what
    forest = pkg.spanning_forest(pairs, n, rec["jaccard"])
    ctx = raw_forest(sel, -np.inf)
    assert forest["edges"].tobytes() == ctx["edges"].tobytes() and np.array_equal(forest["labels"], ctx["labels"]), what
    assert forest["n_edges"] == ctx["n_edges"] and forest["rounds"] == ctx["rounds"], what


def test_graph_calls_share_scratch_across_database_sizes(oracle, grid_hook):
    with Selector(0) as sel:
        rec, cuts, want = load(sel, oracle, SMALL)
        first = leg(sel, cuts, want, "first leg")
        grid_hook(1)                                                                      # the grid-stride paths, at this size
        assert leg(sel, cuts, want, "first leg, one block") == first
        grid_hook(0)
        free_standing(sel, rec, "behind the first leg")
        rec_large, cuts_large, want_large = load(sel, oracle, LARGE)
        leg(sel, cuts_large, want_large, "second leg")
        free_standing(sel, rec_large, "behind the second leg")
        again, cuts_again, want_again = load(sel, oracle, SMALL)                          # buffers larger than needed, full of the other set's values
        assert np.array_equal(np.sort(again), np.sort(rec)) and cuts_again == cuts          # (the same list, in whatever order the pass appended it)
        assert leg(sel, cuts_again, want_again, "third leg") == first
        free_standing(sel, again, "behind the third leg")
