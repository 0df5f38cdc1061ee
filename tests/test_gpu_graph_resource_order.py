"""The order in which a run of a gate graph looks at what its constructor nodes need at run time (spf_amd/csrc/spf_graph.hpp): the
LWE weight slots, then the polynomial weight slots, then the GLWE keyswitch keys — all three before anything is enqueued — and the
public functional keyswitch key at the head of the enqueue.  One graph needs one of each and has none; every load moves the refusal
on to the next resource, with that resource's own text.  Every run fails before a launch, so no bootstrap key is needed."""
import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import ValueKind
from tests import glwe_poly_cases as GC
from tests.pbs_graph_cases import NO_KEY, engine_params

pytestmark = pytest.mark.gpu

LIN_SLOT, POLY_SLOT, KSK_SLOT = 5, 6, 7


def refusal(g, n_nodes) -> str:
    with pytest.raises(spf_amd.SpfError) as e:
        g.run()
    assert e.value.status == NO_KEY, str(e.value)
    assert g.stats()["nodes"] == n_nodes
    return str(e.value)


def test_a_run_names_the_first_missing_resource_in_the_order_of_the_checks():
    P = O.DEFAULT_128.replace(lwe_n=12)         # the tuned context of the graph tests (pbs_graph_cases.keys_of)
    eng = spf_amd.Engine(engine_params(P))
    try:
        rng = np.random.default_rng(0x0D3)
        g = spf_amd.FheCircuit(eng)
        lwe = g.add_input(ValueKind.LWE1, rng.integers(0, 1 << 64, P.k * P.N + 1, dtype=np.uint64))
        glwe = g.add_input(ValueKind.GLWE1, rng.integers(0, 1 << 64, (P.k + 1) * P.N, dtype=np.uint64))
        # added against the order of the checks: the order below is the run's, not the graph's
        nodes = [g.add_public_functional_keyswitch([lwe]), g.add_glwe_keyswitch(KSK_SLOT, glwe)]
        nodes += g.add_glwe_poly_linear(POLY_SLOT, [glwe], 1) + g.add_lwe_linear(LIN_SLOT, [lwe], 1)
        outs = [g.add_output(n, ValueKind(kind)) for n, kind in zip(nodes, (ValueKind.GLWE1, ValueKind.GLWE1, ValueKind.GLWE1, ValueKind.LWE1))]
        n_nodes = g.stats()["nodes"]
        assert n_nodes == 6

        assert f"no weights loaded in slot {LIN_SLOT}" in refusal(g, n_nodes)
        eng.load_lwe_linear_weights(LIN_SLOT, np.array([[3]], dtype=np.int64))
        assert f"no polynomial weights loaded in slot {POLY_SLOT}" in refusal(g, n_nodes)
        eng.load_glwe_poly_weights(POLY_SLOT, GC.csr([[[(1, 2)]]], 1, 1), None, shape=(1, 1))
        assert f"no GLWE keyswitch key loaded in slot {KSK_SLOT}" in refusal(g, n_nodes)
        key = rng.integers(0, 1 << 64, (P.k, P.tr_count, P.k + 1, P.N), dtype=np.uint64)
        eng.load_glwe_keyswitch_key_std(KSK_SLOT, key, P.tr_radix_log, P.tr_count)     # (the context's own radix: a kernel serves it)
        assert "public functional keyswitch key not loaded" in refusal(g, n_nodes)

        assert all(not o.any() for o in outs), "a refused run wrote an output"
        g.close()
    finally:
        eng.close()
