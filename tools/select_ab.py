"""Bit-for-bit A/B of the selection step operators between two builds of the library, on one GPU.

    python tools/select_ab.py --against <libfaceformer_hip.so of the other build> [--timeout 300]

The same seeded inputs go through ff_beam_select, ff_beam_constrained_select, ff_pointer_constrained,
ff_pointer_constrained_ahead, ff_pointer_sample and ff_pointer_forced of both libraries (FF_HIP_LIB selects the build), each
library in a fresh child process under its own `timeout -k 10`; the tool stops at the first non-zero exit status.  Every output
array -- the logits masked in place, the records, the byte rows, the appended rows with their statistics, the counter -- is then
compared byte for byte.  Exit status 0: every array equal.

Shapes, the smallest that reach every branch: ntok = 4; S in {5, 64, 65, 260} (L = 1, 60, 61, 256: one visited word, two, eight,
and a 64-key chunk boundary); W in {1, 3, 8}; two wireframes, kv_len below S on the first, a padding mask on both (fill "all":
the second one is padded out, so its rows have no live key at all); three groups per launch (two on the first wireframe: the
launch's one block is partly empty); per group one finished and one empty beam (W = 1: group 0 finished, group 1 empty); a
sparse follow table in which the edge that row 0 stands on has no successor (a dead end under CONNECT); flags NO_REPEAT,
CONNECT and both; look-ahead budgets 0 and 3; E = 64 with rows and statistics."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NTOK, E, GROUPS, GPW, TERM = 4, 64, 3, 2, (1, 4)
NO_REPEAT, CONNECT = 1, 2


def cases():
    for S in (5, 64, 65, 260):
        for W in (1, 3, 8):
            if W > S:
                continue
            for flags in (NO_REPEAT, CONNECT, NO_REPEAT | CONNECT):
                for fill in ("some", "all"):
                    yield S, W, flags, fill


def inputs(S, W, flags, fill, dev):
    import torch
    g = torch.Generator().manual_seed(1000 * S + 10 * W + flags + (100000 if fill == "all" else 0))
    L, B = S - NTOK, GROUPS * W
    fw = (L + 31) // 32
    rnd = lambda *shape: torch.rand(*shape, generator=g)
    x = {"logits": (rnd(B, S) * 8 - 4), "memory": rnd(2, S, E) - 0.5}
    mask = (rnd(2, S) < 0.15).to(torch.uint8)
    mask[:, TERM[0]] = 0                                     # (one terminator stays live on a wireframe that is not padded out)
    if fill == "all":
        mask[1] = 1
    x["mask"], x["kv_len"] = mask, torch.tensor([S - 1, S], dtype=torch.int32)
    # state: beam 0 of every group live; with W >= 3 beam 1 finished and beam 2 empty, with W = 1 group 0 finished, group 1 empty
    scores, fin = -rnd(B), torch.zeros(B, dtype=torch.int32)
    for grp in range(GROUPS):
        if W >= 3:
            fin[grp * W + 1] = 1
            scores[grp * W + 2] = float("-inf")
    if W == 1:
        fin[0], scores[1] = 1, float("-inf")
    x["scores"], x["fin"], x["dead"] = scores, fin, (rnd(B) < 0.2).to(torch.int32)
    first = torch.randint(-1, L, (B,), generator=g, dtype=torch.int32)
    prev = torch.where(first >= 0, torch.randint(0, L, (B,), generator=g, dtype=torch.int32), torch.full((B,), -1, dtype=torch.int32))
    vis = torch.zeros(B, max(fw, 1) * 32, dtype=torch.bool)
    vis[:, :L] = rnd(B, L) < 0.3
    follows = rnd(2, L, L) < (0.08 if L > 8 else 0.5)
    # the dead end: the first live row of the launch stands on an open loop whose last edge has no successor
    live = 0 if W > 1 else 2
    first[live], prev[live] = 0, L - 1
    follows[:, L - 1, :] = False
    bits = lambda b: (b.reshape(*b.shape[:-1], -1, 32).to(torch.int64) << torch.arange(32)).sum(-1).to(torch.int32)
    pad = torch.zeros(2, L, max(fw, 1) * 32, dtype=torch.bool)
    pad[:, :, :L] = follows
    x["first"], x["prev"], x["visited"], x["follows"] = first, prev, bits(vis)[:, :fw].contiguous(), bits(pad)[:, :, :fw].contiguous()
    x["close_dist"] = torch.randint(0, 6, (2, L, L), generator=g, dtype=torch.uint8)
    x["cycle_len"] = torch.randint(0, 6, (2, L), generator=g, dtype=torch.uint8)
    x["hist"] = torch.randint(0, S, (3, B), generator=g, dtype=torch.int32)
    x["uniforms"], x["forced"] = rnd(B), torch.randint(0, S, (B,), generator=g, dtype=torch.int32)
    return {k: v.to(dev) for k, v in x.items()}


def child(path):
    import torch
    from faceformer_amd.hip import lib, ops
    dev, res = "cuda", {}

    def keep(tag, logits, out, counter, extra=()):
        torch.cuda.synchronize()
        for k, v in list(out.items()) + [("logits", logits), ("counter", counter)] + list(extra):
            res["%s/%s" % (tag, k)] = v.cpu().numpy()

    for S, W, flags, fill in cases():
        x = inputs(S, W, flags, fill, dev)
        tag = "S%d W%d flags%d %s" % (S, W, flags, fill)
        common = dict(memory=x["memory"], mask=x["mask"], kv_len=x["kv_len"], term_range=TERM, want_rows=True)
        cnt = lambda: torch.zeros(1, dtype=torch.int32, device=dev)
        if flags == NO_REPEAT:    # (the operators without the rule: once per shape)
            lg, c, hist = x["logits"].clone(), cnt(), x["hist"].clone()
            keep(tag + "/beam_select", lg, ops.beam_select(lg, x["scores"], x["fin"], W, groups_per_wireframe=GPW, hist=hist, t=2,
                                                           counter=c, ge_bound=NTOK, **common), c, [("hist", hist)])
            lg, c = x["logits"].clone(), cnt()
            keep(tag + "/pointer_sample", lg, ops.pointer_sample(lg, x["uniforms"], temperature=0.8, top_k=3, top_p=0.9, fin=x["fin"],
                                                                 seqs_per_group=GPW * W, want_stats=True, counter=c, ge_bound=NTOK,
                                                                 **common), c)
            lg = x["logits"].clone()
            keep(tag + "/pointer_forced", lg, ops.pointer_forced(lg, x["forced"], memory=x["memory"], mask=x["mask"], kv_len=x["kv_len"],
                                                                 seqs_per_group=GPW * W, want_rows=True, want_stats=True), cnt())
        rule = dict(follows=x["follows"], want_stats=True, **common)
        lg, c = x["logits"].clone(), cnt()
        keep(tag + "/beam_constrained_select", lg,
             ops.beam_constrained_select(lg, x["scores"], x["fin"], x["dead"], x["first"], x["prev"], x["visited"], W, flags, NTOK,
                                         groups_per_wireframe=GPW, counter=c, **rule), c)
        lg, c = x["logits"].clone(), cnt()
        keep(tag + "/pointer_constrained", lg,
             ops.pointer_constrained(lg, x["fin"], x["first"], x["prev"], x["visited"], flags, NTOK, seqs_per_group=GPW * W, counter=c,
                                     **rule), c)
        if flags & CONNECT:
            for budget in (0, 3):
                lg, c = x["logits"].clone(), cnt()
                keep(tag + "/pointer_constrained_ahead budget%d" % budget, lg,
                     ops.pointer_constrained_ahead(lg, x["fin"], x["first"], x["prev"], x["visited"], flags, NTOK, x["follows"],
                                                   x["close_dist"], x["cycle_len"], budget, seqs_per_group=GPW * W, counter=c,
                                                   **common, want_stats=True), c)
    np.savez(path, **res)
    print("%s: %d arrays of %d launches" % (lib.LIB_PATH, len(res), len({k.rsplit("/", 1)[0] for k in res})), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--against", metavar="LIB", help="libfaceformer_hip.so of the other build")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", metavar="NPZ", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.against:
        ap.error("--against is required")
    with tempfile.TemporaryDirectory() as tmp:
        got = []
        for name, libpath in (("other", os.path.abspath(args.against)), ("here", None)):
            env = dict(os.environ)
            env.pop("FF_HIP_LIB", None)
            if libpath:
                env["FF_HIP_LIB"] = libpath
            out = os.path.join(tmp, name + ".npz")
            rc = subprocess.call(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", out], env=env)
            if rc:
                print("%s: exit status %d, stopped" % (name, rc))
                return rc
            got.append(np.load(out))
        a, b = got
        differ = sorted(set(a.files) ^ set(b.files))
        differ += [k for k in sorted(set(a.files) & set(b.files))
                   if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
        ops_seen = sorted({k.split("/")[1].split(" ")[0] for k in b.files})
        dead = sum(int(b[k].any()) for k in b.files if k.endswith("/dead_end"))
        print("operators: " + ", ".join(ops_seen))
        print("%d arrays, %d bytes compared; greedy constrained launches with a dead end: %d" % (len(b.files), sum(b[k].nbytes for k in b.files), dead))
        for k in differ:
            print("DIFFERS: " + k)
        print("every array equal" if not differ else "%d arrays differ" % len(differ))
        return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
