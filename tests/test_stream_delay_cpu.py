"""The logic of tests/stream_delay.py that needs no GPU: where a stage gets its holds, the calibration arithmetic and its clamp, the
"hold too short" refusal, `compare` on CPU tensors, and the discovery wrapper on a scripted `hip._stream` -- alone, under an exception
and together with the host-only harness of tools/launch_trace.py, which replaces `hip._stream` as well."""
import importlib.util
import os

import pytest
import torch

from tests import stream_delay as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def test_a_training_stage_is_held_in_front_of_forward_and_backward():
    assert SD.schedule("train_main") == ("forward", "backward") and SD.schedule("train_policy") == ("forward", "backward")


def test_a_forward_only_stage_is_held_in_front_of_the_forward():
    for stage in ("nograd_train", "eval_masked", "eval_skipping"):
        assert SD.schedule(stage) == ("forward",)
    with pytest.raises(ValueError, match="unknown stage"):
        SD.schedule("train")


# ---- calibration ---------------------------------------------------------------------------------------------------------------------
def test_a_hold_is_twice_the_step_up_to_the_clamp():
    assert SD.hold_ms_for(10.0) == 20.0 and SD.hold_ms_for(124.0) == 248.0
    assert SD.hold_ms_for(125.0) == 250.0 and SD.hold_ms_for(900.0) == SD.MAX_HOLD_MS == 250.0
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            SD.hold_ms_for(bad)


def test_the_step_time_is_the_shortest_measured_step():
    assert SD.step_time([311.9, 134.3]) == 134.3 and SD.step_time([7.4]) == 7.4
    with pytest.raises(ValueError, match="no measured step"):
        SD.step_time([])


def test_calibration_arithmetic():
    rate = SD.rate_from(8000000, 80.0)                       # 8 M cycles took 80 ms: 100 k cycles per ms
    assert rate == 100000.0
    assert SD.units_for(20.0, rate) == 2000000
    assert SD.units_for(0.0, rate) == 1 and SD.units_for(-5.0, rate) == 1          # never an empty launch
    assert SD.units_for(1e9, rate) == SD.units_for(SD.MAX_HOLD_MS, rate) == 25000000       # bounded whatever is asked for
    assert SD.units_for(3.0, SD.rate_from(16, 4.0)) == 12                           # the torch.mm fallback counts launches
    for units, ms in ((0, 1.0), (100, 0.0), (100, -1.0), (100, float("nan"))):
        with pytest.raises(ValueError, match="calibration"):
            SD.rate_from(units, ms)
    with pytest.raises(ValueError):
        SD.units_for(1.0, 0.0)


def test_a_hold_that_came_out_short_fails_its_row():
    SD.check_hold(30.0, 20.0)
    SD.check_hold(45.0, 20.0)
    for measured in (29.9, 0.0, float("nan")):
        with pytest.raises(AssertionError, match="hold too short: row x"):
            SD.check_hold(measured, 20.0, "row x")
    # the clamp can make the factor 2 unreachable; it must not make a short hold pass
    with pytest.raises(AssertionError, match="hold too short"):
        SD.check_hold(SD.hold_ms_for(200.0), 200.0)


# ---- compare -------------------------------------------------------------------------------------------------------------------------
def _outputs():
    return {"logits": torch.arange(6.0).view(2, 3), "decisions": torch.ones(2, 2, 2), "g.w": torch.full((4,), 0.5), "p.w": torch.zeros(4),
            "s.bn.num_batches_tracked": torch.tensor(3)}


def test_compare_finds_nothing_in_equal_outputs():
    assert SD.compare(_outputs(), _outputs()) == []
    nan = {"x": torch.tensor([float("nan"), 1.0])}
    assert SD.compare(nan, {"x": nan["x"].clone()}) == []                            # bits, not values
    assert SD.compare({"x": torch.tensor([0.0])}, {"x": torch.tensor([-0.0])}) == ["x"]


def test_compare_reports_the_differing_keys_in_order():
    got = _outputs()
    got["g.w"][3] += 2.0 ** -20
    got["s.bn.num_batches_tracked"] += 1
    assert SD.compare(_outputs(), got) == ["g.w", "s.bn.num_batches_tracked"]
    with pytest.raises(AssertionError, match=r"row \[train_main\]: with the stream of 2: adamml_dwconv_fwd held, step 1 differs .* in 2 "
                                             r"tensors: g.w, s.bn.num_batches_tracked"):
        SD.assert_same(_outputs(), got, "row [train_main]", 1, "2: adamml_dwconv_fwd")


def test_compare_reports_a_missing_and_an_extra_key_and_other_shapes():
    got = _outputs()
    del got["decisions"]
    got["g.v"] = torch.zeros(1)
    got["p.w"] = torch.zeros(2, 2)
    got["logits"] = got["logits"].double()
    assert SD.compare(_outputs(), got) == ["logits", "missing:decisions", "p.w", "extra:g.v"]


def test_clones_come_back_under_their_keys_with_their_shapes_and_types():
    src = {"logits": torch.arange(6.0).view(2, 3), "s.n": torch.tensor(3), "g.w": torch.full((2, 2, 1), 0.5), "s.m": torch.tensor([7, 8]),
           "p.view": torch.arange(12.0).view(3, 4)[:, 1:3]}                          # (a non-contiguous view is read through its strides)
    keep = SD.Clones()
    for k in ("logits", "s.n", "g.w"):
        keep.add(k, src[k])
    assert keep.enqueue() == ["logits", "s.n", "g.w"]
    want = {k: v.clone() for k, v in src.items()}
    src["logits"].zero_()                                                            # what was enqueued is a copy of the values of then
    keep.add("s.m", src["s.m"])
    keep.add("p.view", src["p.view"])
    assert keep.enqueue() == ["s.m", "p.view"]
    got = keep.read()
    assert set(got) == set(want) and SD.compare(want, got) == []
    assert got["s.n"].dim() == 0 and got["s.n"].dtype == torch.int64 and got["g.w"].shape == (2, 2, 1)


def test_the_report_table_has_one_line_per_row():
    rows = [("rgb_sound", "train_main", "nobody (undelayed)", "-", 41.26, 0), ("rgb_sound", "train_main", "1: adamml_conv_stem1_fwd", 83.04, 41.26, 0)]
    lines = SD.report_table(rows).splitlines()
    assert len(lines) == 4 and lines[0].count("|") == lines[1].count("|") == lines[2].count("|") == 7
    assert lines[2] == "| rgb_sound | train_main | nobody (undelayed) | - | 41.3 | 0 |"
    assert lines[3] == "| rgb_sound | train_main | 1: adamml_conv_stem1_fwd | 83.0 | 41.3 | 0 |"


# ---- discovery -----------------------------------------------------------------------------------------------------------------------
def _scripted(monkeypatch, handles):
    """`hip._stream` returning `handles` one after the other; returns the stand-in, to compare identities with."""
    from adamml_amd import hip
    script = iter(handles)

    def fake_stream():
        return next(script)

    monkeypatch.setattr(hip, "_stream", fake_stream)
    return fake_stream


def test_discovery_names_a_stream_by_its_first_entry_point(monkeypatch):
    from adamml_amd import hip
    fake = _scripted(monkeypatch, [7, 7, 9, 0, 9, 0, 7])
    for name in ("adamml_a", "adamml_b", "adamml_c", "adamml_d"):
        monkeypatch.setitem(hip._fns, name, lambda *args: 0)                         # hip.call's own frame is what the wrapper reads
    with SD.discover() as found:
        hip.call("adamml_a", 1, 2)               # 7
        hip.call("adamml_b")                     # 7 again
        assert hip._stream() == 9                # asked for outside `call` (hip.scratch, a plan replay): seen, not yet named
        assert found.role(9) == "(no launch)"
        hip.call("adamml_c")                     # 0: the default stream
        hip.call("adamml_d")                     # 9: named by its first launch
        hip.call("adamml_a")                     # 0
        hip.call("adamml_d")                     # 7
        assert hip._stream is not fake
    assert hip._stream is fake
    assert found.handles() == [7, 9, 0] and len(found) == 3
    assert found.role_list() == ["adamml_a", "adamml_d", "adamml_c"]
    assert found.entry(1) == (9, "adamml_d")
    found.add(9, "prefetch stream")              # known already: keeps its role
    found.add(11, "prefetch stream")
    assert found.entry(1) == (9, "adamml_d") and found.entry(3) == (11, "prefetch stream")


def test_discovery_goes_on_into_a_given_record(monkeypatch):
    from adamml_amd import hip
    _scripted(monkeypatch, [3, 4, 3, 5])
    monkeypatch.setitem(hip._fns, "adamml_a", lambda *args: 0)
    found = SD.Found()
    with SD.discover(found) as f:
        assert f is found
        hip.call("adamml_a")
        hip._stream()
    with SD.discover(found):
        hip._stream()
        hip.call("adamml_a")
    assert found.handles() == [3, 4, 5] and found.role_list() == ["adamml_a", "(no launch)", "adamml_a"]


def test_the_stream_accessor_is_restored_after_an_exception(monkeypatch):
    from adamml_amd import hip
    fake = _scripted(monkeypatch, [1, 2])
    with pytest.raises(RuntimeError, match="inside the warm-up"):
        with SD.discover() as found:
            hip._stream()
            raise RuntimeError("inside the warm-up")
    assert hip._stream is fake and found.handles() == [1]


@pytest.fixture(scope="module")
def launch_trace():
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    import adamml_amd.runtime  # noqa: F401  (what `_patched` patches is loaded)
    return lt


def test_discovery_inside_the_launch_trace_harness(monkeypatch, launch_trace):
    """tools/launch_trace.py replaces `hip._stream` by a constant 0; discovery entered inside it sees that handle and puts the harness's
    stand-in back, the harness then the accessor it found."""
    from adamml_amd import hip
    fake = _scripted(monkeypatch, [])
    with launch_trace._patched([]):
        stand_in = hip._stream
        assert stand_in is not fake and stand_in() == 0
        with SD.discover() as found:
            buf = hip.scratch(64, torch.device("cpu"))          # the per-stream scratch asks for the stream, as at every launch
            assert buf.numel() * 4 >= 64
        assert hip._stream is stand_in
    assert hip._stream is fake
    assert found.handles() == [0] and found.role_list() == ["(no launch)"]


def test_the_launch_trace_harness_inside_discovery(monkeypatch, launch_trace):
    from adamml_amd import hip
    fake = _scripted(monkeypatch, [21, 22])
    with SD.discover() as found:
        wrapper = hip._stream
        assert hip._stream() == 21
        with launch_trace._patched([]):
            assert hip._stream is not wrapper and hip._stream() == 0      # the harness's constant: not a stream of the step
        assert hip._stream is wrapper and hip._stream() == 22
    assert hip._stream is fake and found.handles() == [21, 22]
