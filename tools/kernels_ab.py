"""What the launch-by-launch A/B tools (vae_kernels_ab.py, step_kernels_ab.py) share: the timed-launch loop and the row format of `run`,
and `compare`.

compare: exits non-zero unless (a) every digest is the same in all files and (b) for every row this tree's median is at most the parent's
median plus the parent's own (max - min), both over the counted launches of all of an arm's runs."""
import hashlib
import statistics
import sys

ROUNDS = 9


def counted(call):
    """one warm-up, then ROUNDS launches with HIP events around each -> (the last result, the times in ms)"""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = call()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return out, ms


def row(key, tensors, ms):
    """print one case: the sha256 over the bytes of the tensor(s), and the times"""
    import torch
    h = hashlib.sha256()
    for t in tensors if isinstance(tensors, (tuple, list)) else (tensors,):
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    print("\t".join(("case", key, h.hexdigest(), " ".join(f"{v:.4f}" for v in ms))), flush=True)


def read(paths):
    """{case: (set of digests, pooled times)} over an arm's files, in the first file's order"""
    rows = {}
    for p in paths:
        for line in open(p):
            if line.startswith("case\t"):
                _, key, digest, ms = line.rstrip("\n").split("\t")
                d, t = rows.setdefault(key, (set(), []))
                d.add(digest)
                t += [float(v) for v in ms.split()]
    return rows


def compare(argv):
    parent, here = read(argv[argv.index("--parent") + 1:argv.index("--here")]), read(argv[argv.index("--here") + 1:])
    n_runs = len(argv) - argv.index("--here") - 1
    print(f"# {len(here)} rows; per arm {n_runs} runs of {ROUNDS} counted launches after one warm-up each, processes alternating; ms: median (min .. max)")
    differ = missed = 0
    if set(parent) != set(here):
        differ += 1
        print(f"DIFFERENT case lists: only in the parent {sorted(set(parent) - set(here))}, only here {sorted(set(here) - set(parent))}")
    for key, (dh, th) in here.items():
        dp, tp = parent.get(key, (set(), [0.0]))
        same = len(dh) == 1 and dh == dp
        bound = statistics.median(tp) + (max(tp) - min(tp))
        ok = statistics.median(th) <= bound
        differ += not same
        missed += not ok
        print(f"{'same bits' if same else 'DIFFERENT'} {'within' if ok else 'MISSED'} {sorted(dh)[0][:12]}  here {statistics.median(th):8.4f} ({min(th):8.4f} .. {max(th):8.4f})  "
              f"parent {statistics.median(tp):8.4f} ({min(tp):8.4f} .. {max(tp):8.4f})  bound {bound:8.4f}  {key}")
    print(f"# (a) bits: {len(here) - differ} of {len(here)} rows equal in every file; (b) time: {len(here) - missed} of {len(here)} rows within their bound")
    if differ or missed:
        sys.exit(f"{differ} row(s) with different bits, {missed} timing row(s) beyond their bound")


def main(run, doc):
    """the command line of an A/B tool: `run`, or `compare --parent FILES --here FILES`"""
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 6 and sys.argv[1] == "compare" and "--parent" in sys.argv and "--here" in sys.argv:
        compare(sys.argv)
    else:
        sys.exit(doc)
