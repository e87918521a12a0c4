"""The host scaffold of the second-order calls (grape_hvp and its halves, grape_hessian, their open-system counterparts; DESIGN.md
28) without a GPU: every driver in csrc/grape_hip.hip goes through one set of helpers -- arguments, prologue, statistics,
reduction, dispatch, extras, residency, info -- and what they replaced is gone, while the sentences a caller can read stayed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _main():
    from grape_jl_amd import api
    return open(os.path.join(api._CSRC, "grape_hip.hip")).read()


def test_arguments_reduction_and_helpers_are_written_once():
    main = _main()
    # the static part of HvpArgs (written as a.H0f / a.s.H0f three times before): closed_series_args alone.  (The evaluation path
    # fills other argument structs -- fa, ea, ta -- from the same field; those are not this family's.)
    assert len(re.findall(r"\ba\.(?:s\.)?H0f = h->d_H0f", main)) == 1
    assert main.count("HvpArgs a{};") == 1
    assert len(re.findall(r"\.ws = nullptr; \w+(?:\.a)?\.tg = nullptr; \w+(?:\.a)?\.stats = nullptr; \w+(?:\.a)?\.rho = nullptr;", main)) == 1   # open_stored_args
    # the H v reduction (over L N_T entries per direction, no z): reduce_directions, nowhere else
    assert len(re.findall(r"grad_reduce_kernel,[^;]*\(int\)LN,[^;]*\(const double2 \*\)nullptr\);", main)) == 1
    for helper in ("HvpArgs closed_series_args(", "LindArgs open_stored_args(", "int second_order_begin(", "int read_stats(",
                   "void reduce_directions(", "void with_np(", "int split_reserve(", "int split_resident(", "void fill_info("):
        assert main.count(helper) == 1, helper
    assert main.count("second_order_begin(h)") == 8                               # the eight drivers
    # one synchronisation per launch group: the reader holds the only one of these drivers besides the final copy of a Hessian
    reader = main[main.index("int read_stats("):main.index("void reduce_directions(")]
    assert reader.count("hipStreamSynchronize") == 1


def test_what_the_helpers_replaced_is_gone():
    main = _main()
    for word in ("HESS_DISPATCH", "hvp_split_stats", "open_hvs_stats", "hess_collect", "hvs_reserve(", "open_hvs_reserve(", "hvp_launch<",
                 "hvp_split_launch_chi", "hvp_split_launch_builtin", "hess_launch_seeds", "hess_launch_backward", "hess_launch_fan"):
        assert word not in main, word
    assert "struct HvpSplit" not in main                                          # neither handle struct: SplitExtras<T> is both
    assert main.count("struct SplitExtras") == 1 and "SplitExtras<double2> hvs;" in main and "SplitExtras<double> hvs;" in main


def test_the_sentences_a_caller_reads_are_unchanged():
    main = _main()
    # the two residency messages: one text in split_resident, the two (call, owner) pairs at its callers
    for piece in ('": nv = " + std::to_string(nv) + " directions do not fit the storage budget of " + owner +',
                  '" (8 GB, half of the free memory, GRAPE_HVP_DIRS): at most " + std::to_string(nd) +',
                  '" stay resident between the halves; loop over groups of that size";',
                  '"grape_hvp_forward", "grape_hvp");', '"grape_open_hvp_forward", "grape_open_hvp");'):
        assert main.count(piece) == 1, piece
    for text in ('"grape_hvp: a series did not converge within 200 terms (direction group starting at "',
                 '"grape_open_hvp: a series did not converge within 200 terms (direction group starting at "',
                 '"grape_hvp_forward: a series did not converge within 200 terms"',
                 '"grape_open_hvp_forward: a series did not converge within 200 terms"',
                 '"grape_hessian: a series did not converge within 200 terms"',
                 '"grape_open_hessian: a series did not converge within 200 terms"'):
        assert main.count(text) == 1, text
    assert main.count('std::string(call) + ": a series did not converge within 200 terms"') == 2   # the backward halves, closed | open
    assert main.count('std::string(call) + ": storage of the split calls: "') == 1
