"""The inputs of tests/test_gpu_sequences.py, checked without a GPU: the scripts never change the time grid, and
at N >= 49 Hermitian -- where the four-product route decides per cell -- every cell keeps ONE route over all pulses of a script,
none of them undecidable, so that no step replays a captured evaluation with another hand-over than it was captured with."""
import numpy as np
import pytest

import sequence_inputs as si
import t16_route_reference as tr


def test_the_scripts_never_change_the_time_grid():
    calls = [c for step in si.SCRIPT for c in step]
    assert not any("tlist" in c for c in calls)
    assert len(si.SCRIPT) == 10 and calls.count("eval") >= 4 + 8 + 12
    assert set(si.GETTERS) <= set(si.SCRIPT[1]) and len(si.GETTERS) == 9
    # the last step crosses the 16th call of the single-wait path and replays after it
    n_eval = 0
    for step in si.SCRIPT[:-1]:
        n_eval += sum(c == "eval" for c in step)
    assert n_eval < 16 < n_eval + len(si.SCRIPT[-1]) - 1


def test_every_case_leaves_a_partial_last_batch_and_order_one_signals():
    for cid, c in si.CASES.items():
        assert c["N_T"] % 16 != 0 and c["N_T"] > 16
        pr = si.problem(cid)
        assert pr["H0"].shape == (c["K"], c["N"], c["N"]) and pr["tlist"].shape == (c["N_T"] + 1,)
        herm = np.abs(pr["H0"] - np.conj(np.swapaxes(pr["H0"], -1, -2))).max() == 0.0
        assert herm == c["herm"], cid
        assert np.abs(np.linalg.norm(pr["target"], axis=1) - 1.0).max() < 1e-14
        x = [si.pulses(cid, i) for i in range(si.N_PULSES)]
        d = [np.abs(x[i] - x[0]).max() for i in range(1, si.N_PULSES)]
        assert 5e-3 < min(d) and max(d) < 6e-2                     # fresh pulses every step, all near x_0
        assert len({xi.tobytes() for xi in x}) == si.N_PULSES


@pytest.mark.parametrize("cid", [c for c, v in si.CASES.items() if v["N"] >= 49 and v["herm"]])
def test_cells_keep_one_route_over_all_pulses_of_a_script(cid):
    pr = dict(si.problem(cid), shape=None)
    first = None
    for i in range(si.N_PULSES):
        dec = tr.decide(tr.with_pulses(pr, si.pulses(cid, i)))
        assert dec["counts"]["undecidable"] == 0, (cid, i, dec["counts"])
        routes = ([list(row) for row in dec["kind"]], dec["sq"].tolist(), dec["skipped"])
        if first is None:
            first = routes
            print(cid, dec["counts"], "plan estimate", float(dec["r"].min()), float(dec["r"].max()),
                  "delta", float(dec["delta"].min()), float(dec["delta"].max()))
            # every cell certified without squarings: the derivative batches take the economized series of the 1.36 segment
            assert dec["counts"]["certified"] == dec["counts"]["ncell"] and dec["counts"]["squarings_kept"] == 0
        assert routes == first, (cid, i)
