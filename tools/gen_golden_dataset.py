#!/usr/bin/env python3
"""Golden frame indices for the dataset loaders (adamml_amd/data.py): calls the REAL reference's sample_train_clip and
sample_val_test_clip (IBM/AdaMML utils/video_dataset.py, imported by path from $ADAMML_REF or the first argument, at generation
time only) over a grid of arguments and records, per row, the arguments, the np.random.seed set just before the call, the indices it
returned (delta-coded) and a digest of numpy's global RNG state right after it -> tests/golden/dataset_index_cases.json.  Nothing from the
reference is copied; the file holds outputs only.  Usage: python tools/gen_golden_dataset.py /path/to/AdaMML"""
import hashlib
import importlib.util
import itertools
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_FRAMES = 8
LENGTHS = (3, 10, 39, 40, 41, 120, 300)


def state_digest():
    """12 hex digits over numpy's global Mersenne Twister state (key and position)."""
    _, key, pos, _, _ = np.random.get_state()
    return hashlib.sha256(np.asarray(key, '<u4').tobytes() + int(pos).to_bytes(4, 'little')).hexdigest()[:12]


def deltas(idx):
    """The indices as their first value followed by the successive differences, a run of three or more equal differences d written
    as the pair [d, count] (the file stays small)."""
    idx = np.asarray(idx).astype(np.int64)
    flat, out, i = [int(idx[0])] + np.diff(idx).tolist(), [], 0
    while i < len(flat):
        j = i
        while j < len(flat) and flat[j] == flat[i]:
            j += 1
        out += [[flat[i], j - i]] if j - i >= 3 else flat[i:j]
        i = j
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ADAMML_REF")
    if not ref:
        raise SystemExit(__doc__)
    spec = importlib.util.spec_from_file_location("reference_video_dataset", os.path.join(ref, "utils", "video_dataset.py"))
    vd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vd)
    warnings.filterwarnings("ignore", category=DeprecationWarning)         # int() of a one-element array in random_clip

    train, val = [], []
    for k, (length, consecutive, freq, dense, clips) in enumerate(itertools.product(LENGTHS, (1, 5), (1, 2), (False, True), (1, 5))):
        np.random.seed(k)
        idx = vd.sample_train_clip(length, consecutive, NUM_FRAMES, freq, dense, clips)
        train.append([[length, consecutive, NUM_FRAMES, freq, dense, clips], k, state_digest(), deltas(idx)])
    for k, (length, consecutive, freq, dense, fixed, clips) in enumerate(
            itertools.product(LENGTHS, (1, 5), (1, 2), (False, True), (False, True), (1, 3, 5, 10))):
        np.random.seed(1000 + k)
        idx = vd.sample_val_test_clip(length, consecutive, NUM_FRAMES, freq, dense, fixed, clips)
        val.append([[length, consecutive, NUM_FRAMES, freq, dense, fixed, clips], 1000 + k, state_digest(), deltas(idx)])
    about = ("Frame indices of the reference's utils/video_dataset.py.  A row is [args, seed, state, deltas]: the positional arguments of "
             "sample_train_clip(video_length, num_consecutive_frames, num_frames, sample_freq, dense_sampling, num_clips) / "
             "sample_val_test_clip(..., dense_sampling, fixed_offset, num_clips); the np.random.seed set just before the call; `deltas`: "
             "the returned 1-based indices as their first value followed by the successive differences, a run of three or more equal "
             "differences d written as [d, count] (indices = cumsum of the expanded list), and `state`: the first "
             "12 hex digits of SHA-256 over numpy's global RNG state after the call (624 key words as little-endian uint32, then the "
             "position as 4 little-endian bytes).")
    path = os.path.join(ROOT, "tests", "golden", "dataset_index_cases.json")
    with open(path, "w") as f:                                             # one line per row
        f.write('{"about": %s,\n "numpy": %s,\n' % (json.dumps(about), json.dumps(np.__version__)))
        for name, rows, last in (("train", train, False), ("val", val, True)):
            f.write(' "%s": [\n%s]%s\n' % (name, ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows), "}" if last else ","))
    print("wrote", path, os.path.getsize(path), "bytes,", len(train), "+", len(val), "rows")


if __name__ == "__main__":
    main()
