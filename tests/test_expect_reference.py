"""Proof of tests/expect_reference.py (no GPU): the einsum reference against long double, against identities, against the
balanced-frame twin of tests/frame_reference.py -- and that the shared comparison ``assert_expect_agrees`` refuses every one of
the deliberately wrong results it has to notice.

Inputs have O(1) signals: ||O_m||_2 = 1, unit-norm states (unit Frobenius norm for density matrices).  Every case asserts on the
reference alone that every observable reaches max_n |e| >= 0.05, so the bound is relative and never its own floor.
"""
import numpy as np
import pytest

import expect_reference as er
import frame_reference as fr
from grape_jl_amd import synth

P = 5   # stored states per trajectory


def closed_case(N, K=3, M=3, per_traj=False, seed=None):
    seed = 40000 + N if seed is None else seed
    fw = synth.unit_vectors(synth.subseed(seed, 1), K * P, N).reshape(K, P, N)
    return fw, er.observables(N, M, seed, K if per_traj else None, non_hermitian=(1,))


def open_case(d, K=2, M=3, per_traj=False, seed=None):
    seed = 50000 + d if seed is None else seed
    z = synth.normal(synth.subseed(seed, 2), 2 * K * P * d * d)
    A = (z[0::2] + 1j * z[1::2]).reshape(K, P, d, d)
    rho = A @ np.conj(np.swapaxes(A, -1, -2))                     # positive, then a non-Hermitian part (a handle stores what the
    rho = rho + 0.1 * np.abs(rho).max() * A / np.abs(A).max()      # caller's rho0 becomes: nothing in the sum assumes symmetry)
    rho = rho / np.sqrt(np.sum(np.abs(rho) ** 2, axis=(-2, -1)))[..., None, None]
    return rho, er.observables(d, M, seed, K if per_traj else None, non_hermitian=(1,))


@pytest.mark.parametrize("N", [5, 17, 64])
@pytest.mark.parametrize("per_traj", [False, True])
def test_closed_double_against_long_double(N, per_traj):
    fw, ops = closed_case(N, per_traj=per_traj)
    want = er.expect_closed(fw, ops, dtype=np.clongdouble)
    er.assert_order_one(want)
    got = er.expect_closed(fw, ops)
    assert got.dtype == np.complex128 and got.shape == (3, P, 3)
    er.assert_expect_agrees(got, want.astype(np.complex128), ops, fw, f"closed N = {N}")
    # written out, one element at a time
    k, n, m = 2, 3, 1
    O = ops[k, m] if per_traj else ops[m]
    assert abs(got[k, n, m] - np.vdot(fw[k, n], O @ fw[k, n])) <= er.bound(ops, fw)[k, n, m]


@pytest.mark.parametrize("d", [4, 17])
@pytest.mark.parametrize("per_traj", [False, True])
def test_open_double_against_long_double(d, per_traj):
    rho, ops = open_case(d, per_traj=per_traj)
    want = er.expect_open(rho, ops, dtype=np.clongdouble)
    er.assert_order_one(want)
    got = er.expect_open(rho, ops)
    er.assert_expect_agrees(got, want.astype(np.complex128), ops, rho, f"open d = {d}")
    k, n, m = 1, 2, 1
    O = ops[k, m] if per_traj else ops[m]
    assert abs(got[k, n, m] - np.trace(O @ rho[k, n])) <= er.bound(ops, rho)[k, n, m]


def test_identity_gives_the_norm_and_the_trace():
    fw, _ = closed_case(17)
    fw = fw * np.array([1.0, 0.5, 2.0])[:, None, None]
    one = np.eye(17)[None]
    got = er.expect_closed(fw, one)
    er.assert_expect_agrees(got, np.sum(np.abs(fw) ** 2, axis=-1)[..., None] + 0j, one, fw, "||Psi||^2")
    rho, _ = open_case(17)
    one = np.eye(17)[None]
    er.assert_expect_agrees(er.expect_open(rho, one), np.trace(rho, axis1=-2, axis2=-1)[..., None], one, rho, "tr rho")


def test_hermitian_operator_gives_a_real_value_inside_the_bound():
    fw, ops = closed_case(64)
    herm = ops[[0, 2]]
    assert np.array_equal(herm, np.conj(np.swapaxes(herm, -1, -2)))
    got = er.expect_closed(fw, herm)
    assert np.all(np.abs(got.imag) <= er.bound(herm, fw))
    assert np.abs(er.expect_closed(fw, ops)[..., 1].imag).max() >= er.MIN_SIGNAL    # (the non-Hermitian one has an imaginary part)


def test_skewed_problem_with_the_congruence_gives_the_twins_values():
    N = 17
    pr = fr.make_twin(N, 2, 2, 4, seed=4117, kind="general")
    e = fr.skew_exponents(N, 4117)
    ops = er.observables(N, 3, 4117, non_hermitian=(1,))
    fw = fr.propagate(pr, pr["pulsevals"], derivatives=False)["fw"]
    fws = fr.propagate(fr.skewed(pr, e), pr["pulsevals"], derivatives=False)["fw"]
    want = er.expect_closed(fw, ops)
    er.assert_order_one(want)
    got = er.expect_closed(fws, er.skewed_ops(ops, e))
    assert np.abs(got - want).max() <= fr.TOL_SCALAR
    # on the twin's own states mapped exactly, the derived bound holds in the skewed frame (the sum is invariant)
    S = 2.0 ** e
    er.assert_expect_agrees(er.expect_closed(fw * S, er.skewed_ops(ops, e)), want, ops, fw, "exact congruence")
    with pytest.raises(AssertionError):
        er.assert_expect_agrees(er.expect_closed(fw * S, er.skewed_ops(ops, e, wrong="similarity")), want, ops, fw, "similarity")


@pytest.mark.parametrize("wrong", er.WRONG)
def test_the_comparison_refuses_a_wrong_closed_result(wrong):
    fw, ops = closed_case(17, per_traj=True)
    want = er.expect_closed(fw, ops)
    er.assert_order_one(want)
    er.assert_expect_agrees(er.expect_closed(fw, ops), want, ops, fw, "control")
    with pytest.raises(AssertionError):
        er.assert_expect_agrees(er.expect_closed(fw, ops, wrong=wrong), want, ops, fw, wrong)


@pytest.mark.parametrize("wrong", [w for w in er.WRONG if w != "bra_not_conjugated"])
def test_the_comparison_refuses_a_wrong_open_result(wrong):
    rho, ops = open_case(17, per_traj=True)
    want = er.expect_open(rho, ops)
    er.assert_order_one(want)
    with pytest.raises(AssertionError):
        er.assert_expect_agrees(er.expect_open(rho, ops, wrong=wrong), want, ops, rho, wrong)


def test_adjoint_of_a_hermitian_operator_is_not_a_mistake():
    """O <-> O^dagger is only visible on a non-Hermitian observable: the refusal above rests on the one every set carries"""
    fw, ops = closed_case(17)
    herm = ops[[0, 2]]
    er.assert_expect_agrees(er.expect_closed(fw, herm, wrong="adjoint"), er.expect_closed(fw, herm), herm, fw, "adjoint of Hermitian")
