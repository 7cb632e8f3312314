"""adamml_amd/prefetch.py without a GPU: with a CPU device the Prefetcher does its look-ahead without streams or events and tensors
pass through, so the ORDER of its calls is checked here -- fetch depth + 1, then one fetch per hand-over; a loader's exception
surfaces at its own batch -- together with the launchers' --prefetch flag and the video.Augmented type."""
import pytest
import torch

from adamml_amd import train, train_unimodal, video as V
from adamml_amd.prefetch import Prefetcher


class Recording:
    """A list-backed loader that writes down what happens: ("iter",), ("fetch", k), and ("raise", k) where batch k raises."""

    def __init__(self, batches, fail_at=None):
        self.batches, self.fail_at, self.log, self.dataset, self.sampler, self.epoch = batches, fail_at, [], "the dataset", "the sampler", 0

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        self.log.append(("iter",))
        self.epoch += 1
        for k, b in enumerate(self.batches):
            if k == self.fail_at:
                self.log.append(("raise", k))
                raise OSError("batch %d cannot be read" % k)
            self.log.append(("fetch", k))
            yield b


def _batches(n, alone=False):
    out = []
    for k in range(n):
        xs = [torch.full((2, 3), float(k)), torch.full((2, 5), 10.0 + k)]
        out.append((xs[0] if alone else xs, torch.tensor([k, k + 1])))
    return out


@pytest.mark.parametrize("depth", [1, 2])
def test_call_order_is_fetch_depth_plus_one_then_one_per_hand_over(depth):
    n = 5
    src = Recording(_batches(n))
    pf = Prefetcher(src, "cpu", depth=depth)
    assert pf.stream is None and len(pf) == n and pf.dataset == "the dataset" and pf.sampler == "the sampler" and pf.epoch == 0
    with pytest.raises(AttributeError):
        pf.no_such_attribute
    for epoch in (1, 2):                                                      # a second iter() starts a new epoch
        src.log.clear()
        it = iter(pf)
        assert src.log == [] or src.log == [("iter",)]                       # (a generator starts at its first next())
        want = [("iter",)]
        for k in range(n):
            inputs, target = next(it)
            fetched = min(n, k + depth + 1)                                   # depth + 1 by the first hand-over, one more by each later one
            want = [("iter",)] + [("fetch", j) for j in range(fetched)]
            assert src.log == want, (k, src.log)
            assert isinstance(inputs, list) and inputs[0] is src.batches[k][0][0] and inputs[1] is src.batches[k][0][1]
            assert target is src.batches[k][1]
        with pytest.raises(StopIteration):
            next(it)
        with pytest.raises(StopIteration):
            next(it)
        assert src.log == want and pf.epoch == epoch
    assert (pf.stats.batches, pf.stats.prepared, pf.stats.late) == (2 * n, 0, 0)
    assert [int(t[0]) for _, t in pf] == list(range(n))                      # and as a plain for loop


def test_fewer_batches_than_the_look_ahead_and_none_at_all():
    src = Recording(_batches(2))
    assert [int(t[0]) for _, t in Prefetcher(src, "cpu", depth=2)] == [0, 1]
    assert list(Prefetcher(Recording([]), "cpu", depth=1)) == []
    with pytest.raises(ValueError, match="depth"):
        Prefetcher(src, "cpu", depth=0)


def test_single_object_batches_come_back_as_single_objects():
    src = Recording(_batches(3, alone=True))
    got = list(Prefetcher(src, "cpu", depth=1))
    assert len(got) == 3
    for k, (x, target) in enumerate(got):
        assert torch.is_tensor(x) and x is src.batches[k][0] and target is src.batches[k][1]


@pytest.mark.parametrize("depth,fail_at", [(1, 2), (2, 2), (2, 0), (1, 4)])
def test_a_loaders_exception_surfaces_at_the_hand_over_of_its_batch(depth, fail_at):
    src = Recording(_batches(5), fail_at=fail_at)
    it = iter(Prefetcher(src, "cpu", depth=depth))
    for k in range(fail_at):                                                  # the batches before it arrive intact
        inputs, target = next(it)
        assert inputs[0] is src.batches[k][0][0] and target is src.batches[k][1]
    assert (("raise", fail_at) in src.log) == (fail_at > 0)                   # raised in the loader already, during the look-ahead
    with pytest.raises(OSError, match="batch %d cannot be read" % fail_at):
        next(it)
    with pytest.raises(StopIteration):                                        # the iterator is dead afterwards
        next(it)
    assert [e for e in src.log if e[0] == "fetch"] == [("fetch", j) for j in range(fail_at)]


def test_frames_on_a_cpu_device_raise_as_require_gpu_does():
    import numpy as np
    g = V.Augmentor(False, 24, disable_scaleup=True).sample(40, 32)
    frames = V.Frames([np.zeros((32, 40, 3), np.uint8)], [g])
    it = iter(Prefetcher([(frames, torch.tensor([0]))], "cpu"))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        next(it)


def test_prefetch_flag():
    p = train.arg_parser()
    assert p.parse_args([]).prefetch == 0
    assert [p.parse_args(["--prefetch", str(n)]).prefetch for n in (0, 1, 2)] == [0, 1, 2]
    with pytest.raises(SystemExit):
        p.parse_args(["--prefetch", "3"])
    a = train.resolve_args(train.arg_parser().parse_args(["--prefetch", "1"]), log=lambda *_: None)
    assert a.prefetch == 1
    u = train_unimodal.resolve_args(train.arg_parser().parse_args(["--prefetch", "1", "--backbone_net", "resnet", "--modality", "rgb"]))
    assert u.prefetch == 1 and u.modality == "rgb"


def test_wrap_leaves_the_loader_alone_without_the_flag_or_without_a_gpu():
    from adamml_amd import prefetch
    src = Recording(_batches(1))
    off = train.arg_parser().parse_args([])
    on = train.arg_parser().parse_args(["--prefetch", "2"])
    assert prefetch.wrap(src, off, "cuda") is src and prefetch.wrap(src, on, "cpu") is src and prefetch.wrap(None, on, "cuda") is None
    assert prefetch.late(src) == 0 and prefetch.late_line(src, 0, 1) is None
    pf = Prefetcher(src, "cpu")
    pf.stats.late = 3
    assert prefetch.late(pf) == 3 and prefetch.late_line(pf, 3, 1) is None and "epoch 7: 2 hand-overs" in prefetch.late_line(pf, 1, 7)


def test_augmented():
    u8 = torch.zeros(2, 8, 8, 24, dtype=torch.uint8)
    a = V.Augmented(u8, "rgb", 24)
    assert a.u8 is u8 and a.modality == "rgb" and a.k_out == 24
    assert a.shape == (2, 8, 8, 24) and a.size() == a.shape and a.size(0) == 2 and a.device == u8.device
    assert a.to("cpu") is a and a.to(torch.device("cpu"), non_blocking=True) is a
    with pytest.raises(ValueError, match="uint8"):
        V.Augmented(u8.float(), "rgb", 24)
    with pytest.raises(ValueError, match="uint8"):
        V.Augmented(u8[0], "rgb", 24)
    with pytest.raises(ValueError, match="uint8"):
        V.Augmented(u8.numpy(), "rgb", 24)
    with pytest.raises(ValueError, match="modality"):
        V.Augmented(u8, "sound", 24)
    with pytest.raises(ValueError, match="k_out"):
        V.Augmented(u8, "rgb", 8)


def test_check_status_raises_decodes_message():
    class Files:                                                              # what check_status reads of an EncodedFrames
        file_of = [(0, 0), (0, 1), (1, 0), (1, 1)]
    V.EncodedFrames.check_status(Files, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"EncodedFrames: video 1, file 0 has a damaged JPEG stream \(decode status 2; 2 files of the batch affected\)"):
        V.EncodedFrames.check_status(Files, torch.tensor([0, 0, 2, 1], dtype=torch.int32))
