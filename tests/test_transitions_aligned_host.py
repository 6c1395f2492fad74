'''Alignment graphs bound to learned transitions, host side: the category of every arc and of
every final state against a map built from (unit name, local source state, local destination
state), for a GraphSet, its SparseGraphs and their dense copies, and the refused cases.  No
device is needed for any of it.'''

import numpy as np
import pytest
import torch

from aligned_truth import CategoryMap, alignment_set, loop_model

from beer_amd.graph import CompiledGraph

TRANSCRIPTIONS = [['s0'], ['s0', 's0'], ['n0', 's1', 's0', 'n0']]


@pytest.fixture(scope='module')
def loop():
    model, units = loop_model(on_host=True)
    return model, units, alignment_set(units, TRANSCRIPTIONS)


def test_every_arc_and_final_state_gets_the_category_of_its_unit(loop):
    model, units, gset = loop
    tmap = CategoryMap(model)
    dense = [g.to_dense() for g in gset]
    for graphs in (gset, list(gset), dense):
        bound = model.bind_alignment_graphs(graphs)
        assert len(bound) == len(TRANSCRIPTIONS)
        for u, seq in enumerate(TRANSCRIPTIONS):
            src, dst, cats, last = tmap.arcs(seq, dense[u])
            assert bound[u] is bound[u]
            assert bound[u].n_states == len(last) == sum(tmap.sizes[name] for name in seq)
            got_src, got_dst = bound[u].arcs
            np.testing.assert_array_equal(got_src, src)
            np.testing.assert_array_equal(got_dst, dst)
            np.testing.assert_array_equal(bound[u].arc_categories, cats)
            np.testing.assert_array_equal(bound[u].final_categories, last)
            assert list(bound[u].pdf_id_mapping) == list(dense[u].pdf_id_mapping)
    # the chains have exactly one final state, and it exits its unit
    for u, seq in enumerate(TRANSCRIPTIONS):
        last = model.bind_alignment_graphs(gset)[u].final_categories
        assert (last >= 0).sum() == 1 and last[-1] == tmap.exit[seq[-1]]
    # a repeated phone shares its categories: [s0, s0] has the arcs of [s0] twice + one exit arc
    one, two = (np.bincount(model.bind_alignment_graphs(gset)[u].arc_categories,
                            minlength=tmap.n_categories) for u in (0, 1))
    want = 2 * one
    want[tmap.exit['s0']] += 1
    np.testing.assert_array_equal(two, want)


def test_fixed_transitions_are_refused(loop):
    _, units, gset = loop
    fixed, _ = loop_model(learned=False, on_host=True)
    with pytest.raises(ValueError, match='not learned'):
        fixed.bind_alignment_graphs(gset)


def test_a_repeated_pdf_id_is_refused(loop):
    _, _, gset = loop
    model, _ = loop_model(on_host=True)
    ids = list(model.graph.pdf_id_mapping)
    ids[1] = ids[0]
    model.graph.pdf_id_mapping = ids
    with pytest.raises(ValueError, match='repeats a pdf id'):
        model.bind_alignment_graphs(gset)


def _edited(dense, edit):
    trans = dense.trans_log_probs.clone()
    edit(trans)
    return CompiledGraph(dense.init_log_probs, dense.final_log_probs, trans,
                         list(dense.pdf_id_mapping))


def test_an_arc_out_of_the_middle_of_a_unit_is_refused(loop):
    model, _, gset = loop
    dense = gset[1].to_dense()                           # [s0, s0]: states 0..2 and 3..5

    def jump(trans):
        trans[1, 3] = np.log(.1)                         # middle state of the first s0 -> the second
    with pytest.raises(ValueError, match='graph 0, arc 1 -> 3'):
        model.bind_alignment_graphs([_edited(dense, jump)])


def test_an_exit_that_branches_is_refused(loop):
    model, _, gset = loop
    dense = gset[2].to_dense()                           # [n0, s1, s0, n0]: s1 = 5..7, s0 = 8..10

    def branch(trans):
        trans[7, 11] = trans[7, 8]                       # the end of s1 -> s0 AND -> the last n0
    with pytest.raises(ValueError, match='two arcs of one category'):
        model.bind_alignment_graphs([_edited(dense, branch)])


def test_an_unbound_graph_still_raises(loop):
    model, _, gset = loop
    # (the model's own E-step entry: what `evidence_lower_bound` and `accumulate_elbo` reach once
    # the frames are on a device; the refusal comes before anything is computed)
    X = torch.zeros(12, 4, dtype=torch.float64)
    for graph in (gset[0], gset[0].to_dense()):
        with pytest.raises(ValueError, match='bind_alignment_graphs'):
            model.expected_log_likelihood(X, inference_graph=graph)
    # ... and so does a graph bound to another model's transitions
    other, _ = loop_model(on_host=True)
    with pytest.raises(ValueError, match='bind_alignment_graphs'):
        model.expected_log_likelihood(X, inference_graph=other.bind_alignment_graphs(gset)[0])
