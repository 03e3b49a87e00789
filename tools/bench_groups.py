"""Grouped-observation export (include/dbg_mi355x_groups.h): observations/s of the device export and of its host copy, on a uniform
read stream and on a poly-A-heavy one, next to the DBG_PATH=generic CountFilterSet time on the same input (the path that does the
same extraction and sort).

    python tools/bench_groups.py [--reads 10000000] [--k 31] [--polya-every 5] [--reps 3] [--out profiles/groups_bench.json]

Poly-A-heavy: every n-th read is replaced by 150 A's (one k-mer then holds reads/n * (150 - k + 1) observations)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dbg = importlib.import_module("rust-debruijn_amd")
capi = importlib.import_module("rust-debruijn_amd._capi")


def timed(fn, reps):
    best = None
    for _ in range(reps + 1):                                   # the first call warms the ctx pools
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--polya-every", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = dbg.Context(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    n, k = a.reads, a.k
    p = dbg.synth_params(n_reads=n, read_len=150, genome_len=n * 150 // 30, error_rate=0.001, stranded=False, n_colours=4)
    nw = lib.dbg_synth_words(C.byref(p))
    pad = 8
    words = torch.zeros(nw + pad, dtype=torch.int64, device=dev)
    start = torch.empty(n, dtype=torch.int64, device=dev)
    length = torch.empty(n, dtype=torch.int32, device=dev)
    colour = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.check(lib.dbg_synth_reads_dev(ctx.h, C.byref(p), words.data_ptr(), start.data_ptr(), length.data_ptr(), colour.data_ptr()))
    start_pa = start.clone()
    start_pa[::a.polya_every] = nw * 32                        # the zero words behind the stream: 150 A's
    inputs = {"uniform": start, "polya": start_pa}
    out = dict(tool="bench_groups", reads=n, read_len=150, k=k, polya_every=a.polya_every, reps=a.reps,
               abi=int(lib.dbg_abi_version()), device=torch.cuda.get_device_name(0))
    for name, st in inputs.items():
        ss = capi.SeqSet(words.data_ptr(), nw + pad, st.data_ptr(), length.data_ptr(), None, colour.data_ptr(), 1, n)
        bounds = (C.c_uint32 * 257)()
        npass = C.c_uint32()
        ctx.check(lib.dbg_kmer_groups_plan_dev(ctx.h, C.byref(ss), k, 0, 0, bounds, C.byref(npass)))
        bl = [int(bounds[i]) for i in range(npass.value + 1)]

        def export(min_export=0):
            parts = []
            for lo, hi in zip(bl[:-1], bl[1:]):
                g = capi.KmerGroups()
                ctx.check(lib.dbg_kmer_groups_dev(ctx.h, C.byref(ss), C.byref(capi.GroupParams(k, 0, lo, hi, min_export, 0)), C.byref(g)))
                parts.append(g)
            return parts

        def free(parts):
            for g in parts:
                lib.dbg_free_groups(ctx.h, C.byref(g))
            parts.clear()

        def timed_export(min_export):
            held = []

            def fn():
                free(held)
                held.extend(export(min_export))
            return timed(fn, a.reps)[0], held

        res = {"passes": npass.value}
        ctx.enable_timing(True)
        t_exp, parts = timed_export(0)
        res["kernel_ms"] = {x["name"]: round(x["ms"], 2) for x in ctx.timings()}
        ctx.enable_timing(False)
        n_obs = sum(g.n_kmer_instances for g in parts)
        res.update(observations=n_obs, groups=sum(g.n for g in parts), export_s=round(t_exp, 4), export_obs_per_s=n_obs / t_exp)
        max_nobs = 0
        hosts = []

        def to_host():
            for h in hosts:
                lib.dbg_free_groups(ctx.h, C.byref(h))
            hosts.clear()
            for g in parts:
                h = capi.KmerGroups()
                ctx.check(lib.dbg_groups_to_host(ctx.h, C.byref(g), C.byref(h)))
                hosts.append(h)
        t_host, _ = timed(to_host, a.reps)
        for h in hosts:
            if h.n:
                arr = (C.c_uint32 * h.n).from_address(h.nobs)
                max_nobs = max(max_nobs, max(arr))
            lib.dbg_free_groups(ctx.h, C.byref(h))
        res.update(host_copy_s=round(t_host, 4), host_copy_obs_per_s=n_obs / t_host, largest_group=int(max_nobs))
        free(parts)
        t_exp2, parts2 = timed_export(2)
        res.update(export_min_obs_2_s=round(t_exp2, 4), exported_obs_min_obs_2=sum(g.n_obs for g in parts2))
        free(parts2)
        with ctx.options(DBG_PATH="generic"):
            def generic():
                t = capi.KmerTable()
                ctx.check(lib.dbg_filter_kmers_dev(ctx.h, C.byref(ss), C.byref(capi.FilterParams(k, 0, 1, 2, 0, 4)), C.byref(t)))
                lib.dbg_free_table(ctx.h, C.byref(t))
            t_gen, _ = timed(generic, a.reps)
        res.update(generic_countfilterset_s=round(t_gen, 4), export_over_generic=round(t_exp / t_gen, 3))
        out[name] = res
        print(name, json.dumps(res), flush=True)
    out["polya_over_uniform"] = round(out["polya"]["export_s"] / out["uniform"]["export_s"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
