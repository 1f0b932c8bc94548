"""CPU: the Tester's report functions on hand-written rows -- every stage's metrics(rows of all ranks) and lines(rows, metrics), with nan
entries, an empty dict and a single pair.  The expected dicts and lines are literals: they were produced once by the code these
functions replaced (main's _print_* helpers with world = 1, recall_metrics, fpfh_metrics and the inline statistics of Tester.test())
on the same rows, and pasted in."""
import math
import warnings

import pytest

nan = float("nan")
BASE = {"IR": 0.4321, "PIR": 0.8765, "pairs": 3, "pairs_without_coarse": 1}
DESC = {0: (0.5, 0.75, 12), 1: (0.0625, 0.25, 3), 3: (0.04, nan, 0)}
DESC_ONE = {7: (0.125, 0.5, 4)}
REG = {0: (1.5, 0.05, 40), 1: (3.25, 0.45, 12), 2: (20.0, 0.1, 7), 5: (0.5, 0.01, 90)}
REG_NAN = {0: (nan, 0.05, 3), 1: (1.0, 0.02, 9)}
REG_ONE = {4: (2.0, 0.25, 11)}
REFINE = {0: (1.5, 0.05, 0.25, 0.01, 0.9, 0.02, 12), 1: (20.0, 0.4, 18.0, 0.35, 0.1, 0.04, 30), 2: (3.0, 0.2, 3.0, 0.2, 0.0, 0.0, 1),
          4: (nan, 0.1, nan, 0.1, 0.5, 0.03, 2)}
STATUS = {0: 16, 1: 0, 2: 12, 4: 3}
REFINE_ONE, STATUS_ONE = {6: (2.0, 0.125, 1.0, 0.0625, 0.75, 0.01, 5)}, {6: 16}
RECALL = {0: (0.5, 0.45, 0.01, True), 1: (0.0, 0.0, nan, False), 2: (0.2, 0.25, 0.5, False), 3: (0.05, 0.07, 0.03, True),
          4: (0.3, 0.3, 0.04, True)}
RECALL_ONE = {2: (0.25, 0.5, 0.0625, False)}
FPFH = {0: (nan, 90.0, 1.5, 0), 1: (0.5, 14.0, 0.31, 20), 2: (0.25, 3.0, 0.1, 50)}
FPFH_ONE = {3: (0.75, 2.0, 0.05, 33)}
LOSSES = {0: (1.5, 1.0, 0.5, 0.0), 1: (nan, 0.75, nan, nan), 2: (2.5, 1.25, 1.25, 0.0)}
LOSSES_ONE = {5: (nan, nan, nan, nan)}
NONRIGID = {0: (0.5, 100), 1: (0.25, 60)}
NONRIGID_ONE = {9: (0.125, 8)}

SUCCESS_NOTE = " (a pose-error success rate, not the 3DMatch-protocol registration recall, which needs the benchmark's gt.info)"


def same(a, b):
    """Equality of nested dicts / lists / numbers where nan equals nan, and a float is not an int."""
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def pose(estimator="compat", refine=None, errors=True):
    from roitr_amd.tester import Pose
    return Pose(estimator, {}, {}, {}, refine, {}, errors)


@pytest.mark.parametrize("rows, metrics, lines", [
    (DESC, {"desc_IR_wo": 0.20083333333333334, "desc_IR_w": 0.5, "desc_FMR": 0.6666666666666666},
     ["[roitr_amd] descriptor matching over 3 pairs: IR without mutual check 0.2008, with 0.5000 (15 mutual matches), FMR at 0.05 0.6667"]),
    (DESC_ONE, {"desc_IR_wo": 0.125, "desc_IR_w": 0.5, "desc_FMR": 1.0},
     ["[roitr_amd] descriptor matching over 1 pairs: IR without mutual check 0.1250, with 0.5000 (4 mutual matches), FMR at 0.05 1.0000"]),
    ({}, {"desc_IR_wo": 0.0, "desc_IR_w": 0.0, "desc_FMR": 0.0}, None)])
def test_descriptor_report(rows, metrics, lines):
    from roitr_amd.tester import DESC_FMR_THRESHOLD, Descriptor
    stage = Descriptor()
    got = stage.metrics(rows, BASE)
    assert same(got, metrics) and DESC_FMR_THRESHOLD == 0.05
    assert stage.lines(rows, {**BASE, **got}) == ({} if lines is None else {"descriptor": lines})


@pytest.mark.parametrize("estimator, rows, lines", [
    ("compat", REG, ["[roitr_amd] registration (compat) over 4 pairs: RRE mean 6.312 deg, median 2.375 deg; RTE mean 0.1525 m, median 0.0750 m",
                     "[roitr_amd] pairs with RRE < 15 deg and RTE < 0.3 m: 0.5000" + SUCCESS_NOTE]),
    ("ransac", REG, ["[roitr_amd] registration (ransac) over 4 pairs: RRE mean 6.312 deg, median 2.375 deg; RTE mean 0.1525 m, median 0.0750 m",
                     "[roitr_amd] pairs with RRE < 15 deg and RTE < 0.3 m: 0.5000" + SUCCESS_NOTE]),
    ("compat", REG_NAN, ["[roitr_amd] registration (compat) over 2 pairs: RRE mean nan deg, median nan deg; RTE mean 0.0350 m, median 0.0350 m",
                         "[roitr_amd] pairs with RRE < 15 deg and RTE < 0.3 m: 0.5000" + SUCCESS_NOTE]),
    ("compat", REG_ONE, ["[roitr_amd] registration (compat) over 1 pairs: RRE mean 2.000 deg, median 2.000 deg; RTE mean 0.2500 m, median 0.2500 m",
                         "[roitr_amd] pairs with RRE < 15 deg and RTE < 0.3 m: 1.0000" + SUCCESS_NOTE]),
    ("compat", {}, None)])
def test_registration_report(estimator, rows, lines):
    stage = pose(estimator)
    merged = {k: (v, None) for k, v in rows.items()}
    assert stage.metrics(merged, BASE) == {}                      # the registration rows add no key to `metrics`
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # numpy's median of a column with a nan
        assert stage.lines(merged, BASE) == ({} if lines is None else {"registration": lines})


@pytest.mark.parametrize("mode, rows, status, line", [
    ("plane", REFINE, STATUS,
     "[roitr_amd] ICP refinement (point-to-plane) over 4 pairs: RRE mean nan -> nan deg, median nan -> nan deg; RTE mean 0.1875 -> 0.1650 m, "
     "median 0.1500 -> 0.1500 m; mean steps 11.2; pairs: converged 1, too few 1, singular 1, empty 1, non-finite 1"),
    ("point", REFINE, STATUS,
     "[roitr_amd] ICP refinement (point-to-point) over 4 pairs: RRE mean nan -> nan deg, median nan -> nan deg; RTE mean 0.1875 -> 0.1650 m, "
     "median 0.1500 -> 0.1500 m; mean steps 11.2; pairs: converged 1, too few 1, singular 1, empty 1, non-finite 1"),
    ("gicp", REFINE_ONE, STATUS_ONE,
     "[roitr_amd] ICP refinement (generalized, plane-to-plane) over 1 pairs: RRE mean 2.000 -> 1.000 deg, median 2.000 -> 1.000 deg; RTE mean "
     "0.1250 -> 0.0625 m, median 0.1250 -> 0.0625 m; mean steps 5.0; pairs: converged 1, too few 0, singular 0, empty 0, non-finite 0"),
    ("plane", {}, {}, None)])
def test_refinement_report(mode, rows, status, line):
    stage = pose("lgr", refine=mode, errors=False)
    merged = {k: (None, v + (status[k],)) for k, v in rows.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # numpy's median of a column with a nan
        assert stage.lines(merged, None) == ({} if line is None else {"refinement": [line]})


def test_pose_reports_both_and_shows_this_ranks_rows():
    stage = pose("compat", refine="gicp")
    stage.rows = {6: (REG_ONE[4], REFINE_ONE[6] + (STATUS_ONE[6],))}
    assert sorted(stage.lines(stage.rows, BASE)) == ["refinement", "registration"]
    assert stage.attributes() == {"registration": {6: REG_ONE[4]}, "refinement": REFINE_ONE, "refinement_status": STATUS_ONE}
    off = pose("ransac", errors=False)
    off.rows = {0: (None, None)}
    assert off.attributes() == {"registration": None, "refinement": None, "refinement_status": None} and off.lines(off.rows, None) == {}


@pytest.mark.parametrize("rows, line", [
    (NONRIGID, "[roitr_amd] 4DMatch non-rigid evaluation over 2 pairs: NFMR 0.3750 (recall threshold 0.04 m, 160 metric points), IR 0.4321 at 0.1 m"),
    (NONRIGID_ONE, "[roitr_amd] 4DMatch non-rigid evaluation over 1 pairs: NFMR 0.1250 (recall threshold 0.04 m, 8 metric points), IR 0.4321 at 0.1 m"),
    ({}, None)])
def test_nonrigid_report(rows, line):
    from roitr_amd.tester import Nonrigid
    stage = Nonrigid(kw={}, radius=0.1)
    assert stage.metrics(rows, BASE) == {} and stage.lines(rows, BASE) == ({} if line is None else {"nonrigid": [line]})
    stage.rows = rows
    assert stage.attributes() == {"nonrigid": rows or None}


RECALL_EMPTY = {"RR": nan, "RR_pairs": 0, "pairs_without_overlap": 0, "RR_overlap_ge_0.3": nan, "RR_overlap_ge_0.3_pairs": 0,
                "RR_overlap_0.1_0.3": nan, "RR_overlap_0.1_0.3_pairs": 0, "RR_overlap_lt_0.1": nan, "RR_overlap_lt_0.1_pairs": 0}


@pytest.mark.parametrize("rows, metrics, line", [
    (RECALL, {"RR": 0.75, "RR_pairs": 4, "pairs_without_overlap": 1, "RR_overlap_ge_0.3": 1.0, "RR_overlap_ge_0.3_pairs": 2,
              "RR_overlap_0.1_0.3": 0.0, "RR_overlap_0.1_0.3_pairs": 1, "RR_overlap_lt_0.1": 1.0, "RR_overlap_lt_0.1_pairs": 1},
     "[roitr_amd] registration recall (RMSE <= 0.2 m, overlap radius 0.0375 m) 0.7500 over 4 pairs (1 without overlap left out); overlap >= 0.3: "
     "1.0000 (2), 0.1 .. 0.3: 0.0000 (1), < 0.1: 1.0000 (1)"),
    (RECALL_ONE, {"RR": 0.0, "RR_pairs": 1, "pairs_without_overlap": 0, "RR_overlap_ge_0.3": nan, "RR_overlap_ge_0.3_pairs": 0,
                  "RR_overlap_0.1_0.3": 0.0, "RR_overlap_0.1_0.3_pairs": 1, "RR_overlap_lt_0.1": nan, "RR_overlap_lt_0.1_pairs": 0},
     "[roitr_amd] registration recall (RMSE <= 0.2 m, overlap radius 0.0375 m) 0.0000 over 1 pairs (0 without overlap left out); overlap >= 0.3: "
     "nan (0), 0.1 .. 0.3: 0.0000 (1), < 0.1: nan (0)"),
    ({}, RECALL_EMPTY,
     "[roitr_amd] registration recall (RMSE <= 0.2 m, overlap radius 0.0375 m) nan over 0 pairs (0 without overlap left out); overlap >= 0.3: "
     "nan (0), 0.1 .. 0.3: nan (0), < 0.1: nan (0)")])
def test_recall_report(rows, metrics, line, tmp_path):
    from roitr_amd.tester import Recall, recall_metrics
    assert same(recall_metrics(rows), metrics)
    stage = Recall(overlap_radius=0.0375, gt_dir=None)
    merged = {k: v + (("T_gt", "info", v[0], "T_est"),) for k, v in rows.items()}      # the stage's rows carry the gt row behind
    got = stage.metrics(merged, BASE)
    assert same(got, metrics) and stage.lines(merged, {**BASE, **got}) == {"recall": [line]}
    stage.rows = merged
    assert same(stage.attributes(), {"recall": rows, "gt": {k: ("T_gt", "info", v[0], "T_est") for k, v in rows.items()}})
    there = Recall(overlap_radius=0.0375, gt_dir=str(tmp_path / "gt"))
    assert there.lines(merged, {**BASE, **got}) == {"recall": [line], "gt": [
        f"[roitr_amd] wrote gt.log, gt.info, gt_overlap.log and est.log for {len(rows)} pairs under {tmp_path / 'gt'}"]}
    assert not (tmp_path / "gt").exists()                          # lines() is pure: finish() writes


@pytest.mark.parametrize("rows, metrics, line", [
    (FPFH, {"fpfh_ir": 0.375, "fpfh_rre": 35.666666666666664, "fpfh_rte": 0.6366666666666667, "fpfh_success": 0.3333333333333333, "fpfh_pairs": 3},
     "[roitr_amd] FPFH baseline (compat, radius 0.125 m, max_nn 100) over 3 pairs: IR 0.3750, RRE mean 35.667 deg, RTE mean 0.6367 m, pairs with "
     "RRE < 15 deg and RTE < 0.3 m: 0.3333"),
    (FPFH_ONE, {"fpfh_ir": 0.75, "fpfh_rre": 2.0, "fpfh_rte": 0.05, "fpfh_success": 1.0, "fpfh_pairs": 1},
     "[roitr_amd] FPFH baseline (compat, radius 0.125 m, max_nn 100) over 1 pairs: IR 0.7500, RRE mean 2.000 deg, RTE mean 0.0500 m, pairs with "
     "RRE < 15 deg and RTE < 0.3 m: 1.0000"),
    ({}, {"fpfh_ir": nan, "fpfh_rre": nan, "fpfh_rte": nan, "fpfh_success": nan, "fpfh_pairs": 0},
     "[roitr_amd] FPFH baseline (compat, radius 0.125 m, max_nn 100) over 0 pairs: IR nan, RRE mean nan deg, RTE mean nan m, pairs with "
     "RRE < 15 deg and RTE < 0.3 m: nan")])
def test_fpfh_report(rows, metrics, line):
    from roitr_amd.tester import Fpfh, fpfh_metrics
    assert same(fpfh_metrics(rows), metrics)
    for options in ({}, dict(radius=0.125, max_nn=100, mutual=False)):      # the defaults of fpfh_handle are the line's defaults
        stage = Fpfh(options, pose("compat"))
        got = stage.metrics(rows, BASE)
        assert same(got, metrics) and stage.lines(rows, {**BASE, **got}) == {"fpfh": [line]}
    with pytest.raises(ValueError, match="lgr"):
        Fpfh({}, pose("lgr"))


@pytest.mark.parametrize("rows, validation, lines", [
    (LOSSES, {"PIR": 0.8765, "IR": 0.4321, "pairs": 3, "skipped": {"PIR": 1, "IR": 0, "loss": 1, "c_loss": 0, "f_loss": 1, "o_loss": 1},
              "loss": 2.0, "c_loss": 1.0, "f_loss": 0.875, "o_loss": 0.0},
     ["[roitr_amd] val over 3 pairs: loss 2.0000  c_loss 1.0000  f_loss 0.8750  o_loss 0.0000  PIR 0.8765  IR 0.4321",
      "[roitr_amd] val: pairs left out of a mean because their value is nan: PIR 1, IR 0, loss 1, c_loss 0, f_loss 1, o_loss 1"]),
    (LOSSES_ONE, {"PIR": 0.8765, "IR": 0.4321, "pairs": 1, "skipped": {"PIR": 1, "IR": 0, "loss": 1, "c_loss": 1, "f_loss": 1, "o_loss": 1},
                  "loss": nan, "c_loss": nan, "f_loss": nan, "o_loss": nan},
     ["[roitr_amd] val over 1 pairs: loss nan  c_loss nan  f_loss nan  o_loss nan  PIR 0.8765  IR 0.4321",
      "[roitr_amd] val: pairs left out of a mean because their value is nan: PIR 1, IR 0, loss 1, c_loss 1, f_loss 1, o_loss 1"]),
    ({}, {"PIR": 0.8765, "IR": 0.4321, "pairs": 0, "skipped": {"PIR": 1, "IR": 0, "loss": 0, "c_loss": 0, "f_loss": 0, "o_loss": 0},
          "loss": nan, "c_loss": nan, "f_loss": nan, "o_loss": nan},
     ["[roitr_amd] val over 0 pairs: loss nan  c_loss nan  f_loss nan  o_loss nan  PIR 0.8765  IR 0.4321",
      "[roitr_amd] val: pairs left out of a mean because their value is nan: PIR 1, IR 0, loss 0, c_loss 0, f_loss 0, o_loss 0"])])
def test_validation_report(rows, validation, lines):
    from roitr_amd.tester import Losses
    stage = Losses(config={})
    got = stage.metrics(rows, BASE)
    assert same(got, validation) and stage.publishes == "validation" and stage.lines(rows, got) == {"val": lines}


def test_constants_and_the_order_of_the_printed_lines():
    from roitr_amd import tester as T
    assert (T.SUCCESS_RRE, T.SUCCESS_RTE, T.RECALL_RMSE, T.DESC_INLIER_THRESHOLD) == (15.0, 0.3, 0.2, 0.1)
    assert T.REPORT_ORDER == ("val", "eval", "descriptor", "registration", "fpfh", "refinement", "recall", "gt", "nonrigid")


def test_the_tester_builds_its_stage_list_once_and_takes_the_implied_options():
    from roitr_amd.tester import Tester
    cfg = {"benchmark": "3DMatch"}
    t = Tester(cfg, None, [], gt_dir="somewhere", refine="plane", descriptor_eval=True, validate=True, fpfh_baseline={}, estimator="compat")
    assert [s.name for s in t.stages] == ["losses", "descriptor", "pose", "fpfh", "recall"] and t.evaluate and t.register
    assert (t.losses, t.descriptor, t.registration, t.refinement, t.refinement_status, t.fpfh, t.recall, t.gt) == ({},) * 8
    assert t.nonrigid is None and t.validation is None and t.metrics is None and t.records is None
    t = Tester({"benchmark": "4DMatch"}, None, [], evaluate=True, descriptor_eval=False, fpfh_baseline={})
    assert [s.name for s in t.stages] == ["nonrigid"] and t.fpfh is None and t.fpfh_baseline == {} and not t.register
    t = Tester(cfg, None, [], descriptor_eval=True, register=True)           # descriptor_eval needs evaluate; no RRE / RTE without it
    assert [s.name for s in t.stages] == ["pose"] and t.descriptor is None and t.registration is None and t.refinement is None
    for bad in (dict(estimator="icp"), dict(refine="colored"), dict(estimator="lgr", fpfh_baseline={})):
        with pytest.raises(ValueError):
            Tester(cfg, None, [], **bad)


def test_no_stage_imports_its_module_before_it_runs():
    """A fresh interpreter: building a Tester with every option on, and importing the command line, loads none of the stages' modules."""
    import os
    import subprocess
    import sys
    code = ("import sys; from roitr_amd.tester import Tester; import roitr_amd.main; "
            "Tester({'benchmark': '4DMatch'}, None, [], gt_dir='x', refine='gicp', descriptor_eval=True, validate=True, fpfh_baseline={}, "
            "estimator='compat', voxel_size=0.1, points_lim=100); "
            "sys.exit(int(any('roitr_amd.' + m in sys.modules for m in "
            "('icp', 'gicp', 'lgr', 'compat', 'fpfh', 'pairgt', 'descmatch', 'loss', 'nonrigid', 'prep'))))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
