"""CPU: the two restatements of cnveval.Evaluate (tests/cnveval_ref.py) against each other, and the report's text.

The literal walk is the judge of the device kernels; the order-free form is what the kernels implement.  They must
give the same count in every (sample, class) cell of every case."""
import pytest

from tests import cnveval_ref as R
from tests import cnveval_shapes as S


@pytest.mark.parametrize("name", sorted(S.cases()))
def test_literal_walk_equals_order_free_form(name):
    case = S.cases()[name]
    names, want = S.reference(name)
    got = R.as_array(R.evaluate_order_free(case.cnvs, case.truths, case.po), names)
    assert got == want.tolist()


def test_every_hand_case_counts_something_but_the_empty_ones():
    for name in S.cases():
        _, want = S.reference(name)
        assert (want.sum() > 0) == (name not in ("hand_no_calls", "hand_nothing")), name


def test_worked_example_text():
    names, want = S.reference("hand_worked")
    assert names == ["a", "b", "c"]
    assert want[2].sum() == 0                                    # c has no calls: not even its false negative
    case = S.cases()["hand_worked"]
    assert R.report(R.evaluate_literal(case.cnvs, case.truths, case.po)) == S.WORKED_OUT


def test_hand_cases_pin_what_they_are_named_for():
    FP, FN, TP, TN = R.FP, R.FN, R.TP, R.TN
    ref = lambda n: S.reference("hand_" + n)[1]
    assert ref("exact_2_of_5")[0, 0, TP] == 1 and ref("short_of_2_of_5")[0, 0, FN] == 1
    assert ref("exact_5_of_10")[0, 0].tolist() == [2, 0, 0, 0]  # a's call: uncounted, and an FP under b's truth
    assert ref("short_of_5_of_10")[0, 0].tolist() == [1, 0, 0, 1]
    # abutting: an overlap of 0 matches nothing, so each sample misses its truth; the other sample's truth is its call exactly
    assert ref("abutting").sum(axis=(0, 1)).tolist() == [4, 2, 0, 0]
    assert ref("zero_length_truth").sum(axis=(0, 1))[TP] == 0
    assert ref("cn_3_is_7")[0, 0, TP] == 1 and ref("cn_2_is_not_3").sum(axis=(0, 1))[TP] == 0
    assert ref("cn_negative")[:, 0, TP].tolist() == [1, 0, 0]
    # the counted call is the first in input order: the other one is the false positive, in its own class
    assert ref("tie_input_order")[0, :, FP].tolist() == [0, 1, 0]
    assert ref("tie_input_order_swapped")[0, :, FP].tolist() == [0, 0, 1]
    assert ref("sample_named_twice")[0, 0].tolist()[1:3] == [2, 2]
    assert ref("walk_first_is_own")[0, 0].tolist() == [1, 0, 1, 0]     # nothing added under b's truth, not even a TN
    assert ref("walk_later_own_stops")[0, 0, FP] == 3 + 2
    assert ref("walk_non_matching_inside")[0, 0, FP] == 5 + 4


def test_nan_spelling():
    assert R.stat_string([0, 0, 0, 0]) == "precision: NaN (0    / (0    + 0   )) recall: NaN (0    / (0    + 0   ))"
    assert R.report({}).splitlines()[3] == "size-class: all          | " + R.stat_string([0, 0, 0, 0])


def test_fuzz_small_cases_agree():
    for seed in range(300):
        case = S.seeded(50000 + seed, 1 + seed % 4, seed % 7, 1 + seed % 5, span=60, max_len=40, po=(0.4, 0.5, 1.0)[seed % 3])
        a = R.evaluate_literal(case.cnvs, case.truths, case.po)
        b = R.evaluate_order_free(case.cnvs, case.truths, case.po)
        drop = lambda st: {k: v for k, v in st.items() if any(v)}
        assert drop(a) == drop(b), seed
