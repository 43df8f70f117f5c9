"""CPU: the fold model's inputs discriminate (tests/fold_model.py).

A GPU test that a kernel folding in the wrong order would pass is worthless,
so this pins, on the model alone, that the inputs tests/test_fold_kernel_gpu.py
uses make the three fold orders differ wherever arithmetic lets them:
  * sum on `mixed`: left and tree differ (association shows in the rounding);
  * max / min on `specials`: left, reverse and tree all differ (the result is
    an operand's own bits: NaNs and the two zeros follow the operand order);
  * f16 sum on `specials`: left and reverse differ (the NaN payload follows
    the operand order).
And the facts that bound what any test can tell apart: sum / product on
`mixed` is the same in left and reverse order bit for bit (IEEE
commutativity), so a reverse fold shows only under max / min and the 16-bit
NaN rule; bf16 sum / product on `specials` is 0x7FC0 whatever the order.
"""
import numpy as np
import pytest

import fold_model as fm

N = 4099
ROUNDING = ("f16", "bf16", "f32", "f64", "f8e4m3", "f8e5m2")


def ndiff(a, b):
    return int((fm.bits(a) != fm.bits(b)).sum())


@pytest.mark.parametrize("k", (4, 8))
@pytest.mark.parametrize("dtype", ROUNDING)
def test_sum_on_mixed_tells_left_from_tree(dtype, k):
    srcs = [fm.mixed(dtype, N, np.random.default_rng(5 + j)) for j in range(k)]
    d = ndiff(fm.fold("sum", dtype, srcs, 0), fm.fold("sum", dtype, srcs, 2))
    print(dtype, k, "left vs tree:", d)
    assert d >= 1


@pytest.mark.parametrize("op", ("max", "min"))
@pytest.mark.parametrize("dtype", fm.FLOATS)
def test_max_min_on_specials_tell_all_three_orders_apart(dtype, op):
    rng = np.random.default_rng(5)
    srcs = [fm.specials(dtype, N, rng) for _ in range(4)]
    f = [fm.fold(op, dtype, srcs, m) for m in range(3)]
    print(dtype, op, "0 vs 1:", ndiff(f[0], f[1]), "1 vs 2:", ndiff(f[1], f[2]))
    assert ndiff(f[0], f[1]) >= 1
    assert ndiff(f[1], f[2]) >= 1


def test_f16_sum_on_specials_tells_left_from_reverse():
    rng = np.random.default_rng(5)
    srcs = [fm.specials("f16", N, rng) for _ in range(4)]
    assert ndiff(fm.fold("sum", "f16", srcs, 0), fm.fold("sum", "f16", srcs, 1)) >= 1


@pytest.mark.parametrize("op", ("sum", "product"))
@pytest.mark.parametrize("dtype", fm.DTYPES)
def test_sum_and_product_on_mixed_cannot_tell_left_from_reverse(dtype, op):
    """A fact, not a failure: a op b == b op a bit for bit on these inputs."""
    rng = np.random.default_rng(5)
    srcs = [fm.mixed(dtype, N, rng) for _ in range(5)]
    assert ndiff(fm.fold(op, dtype, srcs, 0), fm.fold(op, dtype, srcs, 1)) == 0


@pytest.mark.parametrize("op", ("sum", "product"))
def test_bf16_sum_and_product_on_specials_are_order_blind(op):
    """Every NaN result is the canonical 0x7FC0, so no order shows."""
    rng = np.random.default_rng(5)
    srcs = [fm.specials("bf16", N, rng) for _ in range(4)]
    f = [fm.fold(op, "bf16", srcs, m) for m in range(3)]
    assert ndiff(f[0], f[1]) == 0 and ndiff(f[1], f[2]) == 0
    nan = (f[0] & 0x7FFF) > 0x7F80
    assert nan.any() and (f[0][nan] == 0x7FC0).all()


@pytest.mark.parametrize("dtype", fm.DTYPES)
def test_tree_of_two_is_left_and_tree_of_one_is_the_source(dtype):
    rng = np.random.default_rng(5)
    for op in fm.ops_of(dtype):
        srcs = fm.inputs(op, dtype, 2, 257, rng)
        assert ndiff(fm.fold(op, dtype, srcs, 2), fm.fold(op, dtype, srcs, 0)) == 0
        for mode in range(3):
            assert ndiff(fm.fold(op, dtype, srcs[:1], mode), srcs[0]) == 0


def test_orders_on_a_hand_made_case():
    """max is (a < b) ? b : a: the first operand on a tie or an unordered pair."""
    nan, one, two = np.float32(np.nan), np.float32(1), np.float32(2)

    def folds(*xs):
        srcs = [np.array([x], np.float32) for x in xs]
        return [fm.fold("max", "f32", srcs, m)[0] for m in range(3)]
    # left: nan, nan, nan.  reverse: (1 ? nan) -> 1, 1, 1.  tree: (nan ? 1) -> nan, (1 ? 1) -> 1, (nan ? 1) -> nan
    left, rev, tree = folds(nan, one, one, one)
    assert np.isnan(left) and rev == one and np.isnan(tree)
    # left: (1 ? nan) -> 1, (1 ? nan) -> 1, (1 ? 2) -> 2.  reverse: (nan ? 1) -> nan, (nan ? nan) -> nan, (2 ? nan) -> 2.
    # tree: (1 ? nan) -> 1, (nan ? 2) -> nan, (1 ? nan) -> 1
    left, rev, tree = folds(one, nan, nan, two)
    assert left == two and rev == two and tree == one
