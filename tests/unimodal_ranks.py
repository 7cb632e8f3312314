"""One rank of tests/test_unimodal_gpu.py::test_two_ranks_end_with_the_same_parameters, started by the test in a fresh process: runs the
unimodal launcher's worker as `--multiprocessing-distributed` rank `gpu` of `world` and leaves a digest of what it ended with."""
import hashlib
import json
import os


def state_digest(model):
    h = hashlib.sha256()
    for k, v in model.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def rank_main(gpu, world, argv, outdir):
    from adamml_amd import train, train_unimodal as TU
    args = TU.resolve_args(train.arg_parser().parse_args(argv))
    args.world_size = world                                   # what train.launch sets before it spawns (one node)
    res = TU.main_worker(gpu, world, args, None, None, lambda *_: None)
    out = {"rank": args.rank, "digest": state_digest(res["model"]), "stats": res["ddp_stats"], "sync": bool(res["model"].rt.sync.enabled),
           "losses": res["history"][0][1]}
    with open(os.path.join(outdir, "rank%d.json" % gpu), "w") as f:
        json.dump(out, f)
