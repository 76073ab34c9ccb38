"""tools/benchkit.py without a device: the schedule of the alternation with a scripted clock in place of the timed window, the
per-side figures, and the reader of a kernel-stats CSV."""
import json

import pytest

from tools import benchkit


def scripted(log, ms):
    """a `window` that records (side, iterations) and answers the next scripted milliseconds of that side"""
    answers = {side: iter(values) for side, values in ms.items()}

    def window(fn, iters):
        log.append((fn.__name__, iters))
        return next(answers[fn.__name__])
    return window


def sides(log):
    def a():
        log.append(("a", "call"))

    def b():
        log.append(("b", "call"))
    return {"a": a, "b": b}


def test_alternate_warms_up_and_calibrates_each_side_then_alternates():
    log = []
    # a: 2 ms per call -> int(50 / 2) + 1 = 26 iterations for a window of 0.05 s; b: 40 ms per call -> 2, floored at calibrate = 3
    clock = scripted(log, {"a": [2.0, 2.11111, 2.33333, 2.22222], "b": [40.0, 40.5, 39.5, 41.25]})
    stats, times = benchkit.alternate(sides(log), 2, 0.05, 3, calibrate=3, digits=4, window=clock)
    assert log == [("a", "call"), ("a", "call"), ("a", 3), ("b", "call"), ("b", "call"), ("b", 3),
                   ("a", 26), ("b", 3), ("a", 26), ("b", 3), ("a", 26), ("b", 3)]
    assert times == {"a": [2.11111, 2.33333, 2.22222], "b": [40.5, 39.5, 41.25]}           # unrounded, for the tool's own comparisons
    assert stats == {"a": {"ms": [2.1111, 2.3333, 2.2222], "median_ms": 2.2222, "min_ms": 2.1111, "max_ms": 2.3333, "iterations_per_window": 26},
                     "b": {"ms": [40.5, 39.5, 41.25], "median_ms": 40.5, "min_ms": 39.5, "max_ms": 41.25, "iterations_per_window": 3}}
    assert list(stats) == ["a", "b"] and list(stats["a"]) == ["ms", "median_ms", "min_ms", "max_ms", "iterations_per_window"]


def test_alternate_keeps_the_tools_constants_apart():
    log = []
    clock = scripted(log, {"a": [0.123456789, 0.123456789, 0.2], "b": [1000.0, 7.0, 9.0]})
    stats, _ = benchkit.alternate(sides(log), 0, 0.5, 2, calibrate=5, digits=5, count_key="calls_per_window", window=clock)
    assert [entry for entry in log if entry[1] != "call"] == [("a", 5), ("b", 5), ("a", 4051), ("b", 5), ("a", 4051), ("b", 5)]
    assert stats["a"] == {"ms": [0.12346, 0.2], "median_ms": 0.16173, "min_ms": 0.12346, "max_ms": 0.2, "calls_per_window": 4051}
    assert stats["b"]["median_ms"] == 8.0 and stats["b"]["calls_per_window"] == 5 and "iterations_per_window" not in stats["b"]
    assert not [entry for entry in log if entry[1] == "call"], "no warm-up was asked for"


def test_window_stats_rounds_every_figure_to_the_digits():
    got = benchkit.window_stats([1.23456, 1.23444, 5.0], 7, 3, "steps_per_window")
    assert got == {"ms": [1.235, 1.234, 5.0], "median_ms": 1.235, "min_ms": 1.234, "max_ms": 5.0, "steps_per_window": 7}
    assert benchkit.window_stats([3.0, 1.0], 1, 4, "n")["median_ms"] == 2.0             # an even count: the mean of the middle two


def test_read_stats_reads_the_four_columns(tmp_path):
    run = tmp_path / "host" / "123"
    run.mkdir(parents=True)
    (run / "x_kernel_stats.csv").write_text('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
                                            '"void sr::k_loss_forward(float const*, int)",50,1500000,30000.5,75.0,29000,31000,1.5\n'
                                            '"k_other",3,500000,166666.7,25.0,1,2,0.1\n')
    (run / "x_kernel_trace.csv").write_text("not the statistics\n")
    assert benchkit.read_stats(str(tmp_path)) == [("void sr::k_loss_forward(float const*, int)", 50, 30000.5, 1500000.0), ("k_other", 3, 166666.7, 500000.0)]


def test_read_stats_without_a_file_ends_the_tool(tmp_path):
    (tmp_path / "kernel_trace.csv").write_text("Name\n")
    with pytest.raises(SystemExit, match="no kernel_stats.csv"):
        benchkit.read_stats(str(tmp_path))


def test_write_doc_writes_and_prints_the_same_document(tmp_path, capsys):
    doc = {"protocol": "p", "a": {"ms": [1.0]}}
    out = tmp_path / "new" / "doc.json"
    benchkit.write_doc(doc, str(out))
    assert json.loads(out.read_text()) == doc and json.loads(capsys.readouterr().out) == doc
    benchkit.write_doc(doc, None)                                                       # no --out: printed only
    assert json.loads(capsys.readouterr().out) == doc
