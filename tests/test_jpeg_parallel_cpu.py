"""The parallel entropy stage for JPEG scans without restart markers, without a GPU: its Python restatement (tests/jpeg_sync_ref.py:
guessed starts, rounds to a fixed point, placement, DC prefix sums) gives the sequential restatement's coefficients on every
marker-less fixture, old and new, within as many rounds as subsequences; the new fixtures (tools/gen_jpeg_parallel_golden.py) have the
properties they were searched for and Pillow's pixels; damaged streams make the stage give the image up; the probe and
`Batch.parallel` answer as documented."""
import hashlib
import os

import numpy as np
import pytest

from adamml_amd import abi, hip, jpeg as J
from tests import jpeg_ref as R, jpeg_sync_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
NEW = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_parallel_cases.npz"))
FILES = {k[:-4]: OLD[k].tobytes() for k in OLD.files if k.endswith(".jpg")}
FILES.update({k[:-6]: OLD[k].tobytes() for k in OLD.files if k.endswith(".frame") and k.startswith("full")})
NEW_NAMES = sorted(k[:-4] for k in NEW.files if k.endswith(".jpg"))
FILES.update({k: NEW[k + ".jpg"].tobytes() for k in NEW_NAMES})
MARKERLESS = sorted(k for k, f in FILES.items() if len(J.parse(f).segments) == 1)


def test_there_are_marker_less_fixtures_of_every_kind():
    assert len(MARKERLESS) >= 20 and set(NEW_NAMES) <= set(MARKERLESS) and "full_256x341" in MARKERLESS
    assert {(i.channels, i.sampling) for i in (J.parse(FILES[k]) for k in NEW_NAMES)} == {(3, 2), (3, 1), (1, 1)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_parallel_cases.npz")) < 300 * 1024


@pytest.mark.parametrize("name", MARKERLESS)
def test_parallel_model_equals_the_sequential_restatement(name):
    b = J.Batch([FILES[name]])
    data, meta = b.data.numpy(), b.meta.numpy()
    want, status = R._entropy(data, meta, meta[:J.DESC])
    got, info = M.entropy(data, meta, meta[:J.DESC])
    print("  %-28s %4d subsequences, %3d rounds, %4d decodes, %3d guesses met a bad code" % (name, info["nsub"], info["rounds"], info["decodes"],
                                                                                           info["unknown"]))
    assert status == 0 and info["eligible"] and not info["gave_up"]
    assert info["nsub"] == -(-(b.infos[0].segments[0][1] - b.infos[0].segments[0][0]) // J.SUBSEQ_BYTES)
    assert 1 <= info["rounds"] <= info["nsub"]
    for c, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (name, c, int((g != w).sum()))


def test_other_subsequence_sizes_reach_the_same_fixed_point():
    """The model at 32, 64 and 256 bytes: the same coefficients, fewer rounds for longer subsequences on the full frame."""
    rounds = {}
    for name in ("full_256x341", "c420_q100_33x47", "noise_grey_q100_96x96"):
        b = J.Batch([FILES[name]])
        data, meta = b.data.numpy(), b.meta.numpy()
        want, _ = R._entropy(data, meta, meta[:J.DESC])
        for S in (32, 256) if name.startswith("full") else (32, 64):
            got, info = M.entropy(data, meta, meta[:J.DESC], subseq=S)
            assert not info["gave_up"] and info["rounds"] <= info["nsub"], (name, S)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, S)
            rounds[name, S] = info["rounds"]
    assert rounds["full_256x341", 256] < rounds["full_256x341", 32]


def test_new_fixtures_have_their_properties_and_pillows_pixels():
    props = {k: M.properties(J.Batch([FILES[k]]), 0) for k in NEW_NAMES}
    for k in NEW_NAMES:
        print("  %-28s %s" % (k, sorted(props[k])))
        px = R.decode(FILES[k])
        if k + ".pixels" in NEW.files:
            assert np.array_equal(px, NEW[k + ".pixels"]), k
        else:
            assert hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == NEW[k + ".sha256"].tobytes(), k
    for k in NEW_NAMES:
        if k.startswith("noise"):
            inf = J.parse(FILES[k])
            assert (inf.height, inf.width) == (96, 96) and "long_chain" in props[k], k
        else:
            assert k[:k.rindex("_seed")] in props[k], k                      # the property the file is named for
    assert {(3, 2), (3, 1), (1, 1)} == {(J.parse(FILES[k]).channels, J.parse(FILES[k]).sampling) for k in NEW_NAMES if k.startswith("noise")}
    assert any("mid_code" in p for p in props.values())
    assert "short" in M.properties(J.Batch([FILES["c420_q93_1x1"]]), 0)
    # the lengths, read off the packed batch itself
    for k, rest in (("len_kS", 0), ("len_kS1", 1)):
        name = [n for n in NEW_NAMES if n.startswith(k + "_seed")][0]
        a, e = J.parse(FILES[name]).segments[0]
        assert (e - a) % J.SUBSEQ_BYTES == rest and e - a > J.SUBSEQ_BYTES
    name = [n for n in NEW_NAMES if n.startswith("ff00_split")][0]
    a, e = J.parse(FILES[name]).segments[0]
    raw = FILES[name][a:e]
    assert any(raw[k - 1] == 0xFF and raw[k] == 0 for k in range(J.SUBSEQ_BYTES, len(raw), J.SUBSEQ_BYTES))


@pytest.mark.parametrize("kind", ["cut", "ff", "zero", "tail0"])
def test_the_stage_gives_a_damaged_stream_up(kind):
    """Whatever the sequential decoder answers with a status, the parallel stage leaves to it."""
    names = ["c420_q93_48x67", "grey_q93_41x30", "noise_grey_q100_96x96", "c444_q93_16x16"]
    b = J.Batch([FILES[k] for k in names])
    for i, name in enumerate(names):
        data, meta = R.damage(b, i, kind)
        desc = meta[i * J.DESC:(i + 1) * J.DESC]
        _, status = R._entropy(data, meta, desc)
        got, info = M.entropy(data, meta, desc)
        assert status != 0 and info["eligible"] and info["gave_up"] and got is None, (kind, name, status)
        assert info["rounds"] <= info["nsub"]
        for j in range(b.n):                                                 # and the others are decoded as ever
            if j != i and j < 2:
                dj = meta[j * J.DESC:(j + 1) * J.DESC]
                assert not M.entropy(data, meta, dj)[1]["gave_up"]


def test_probe_and_batch_parallel_answer_as_documented():
    lib = hip.load()
    probe = lib.adamml_jpeg_decode_parallel_supported
    S = J.SUBSEQ_BYTES
    assert abi.DEFINES["ADAMML_JPEG_SUBSEQ_BYTES"] == S == 128
    assert str(abi.FUNCTIONS["adamml_jpeg_decode_parallel_supported"]) == (
        "int adamml_jpeg_decode_parallel_supported(int H, int W, int components, int sampling, int segments, int64_t coded_bytes)")
    assert probe(256, 341, 3, 2, 1, 44000) == 1 and probe(256, 341, 3, 2, 16, 44000) == 0          # restart markers: today's path
    assert probe(1, 1, 3, 2, 1, 10) == 1 and probe(41, 30, 1, 1, 1, 1154) == 1 and probe(30, 41, 3, 1, 1, 5000) == 1
    assert probe(256, 341, 3, 2, 1, 2048 * S) == 1 and probe(256, 341, 3, 2, 1, 2048 * S + 1) == 0   # the record cap
    assert probe(256, 341, 3, 2, 1, 0) == 0 and probe(256, 341, 3, 2, 0, 100) == 0
    assert probe(0, 341, 3, 2, 1, 100) == 0 and probe(70000, 4, 3, 2, 1, 100) == 0 and probe(16384, 16384, 3, 2, 1, 100) == 0
    assert probe(256, 341, 2, 2, 1, 100) == 0 and probe(256, 341, 3, 3, 1, 100) == 0
    names = ["full_256x341", "full_256x341_rst1", "c420_q93_1x1", "c420_q93_50x70_rst1", "noise_c444_q100_96x96"]
    FILES["full_256x341_rst1"] = OLD["full_256x341_rst1.frame"].tobytes()
    b = J.Batch([FILES[k] for k in names])
    assert b.parallel == [True, False, True, False, True]
    assert "SUBSEQ_BYTES" in J.__all__
    # the ABI around it is unchanged
    assert len(hip.SIGNATURES["adamml_jpeg_decode_u8"]) == 11 and lib.adamml_jpeg_decode_workspace(10) == 1920
