#!/usr/bin/env python3
"""Headline benchmark: mel-frames/s of the whole Inference_Step (encoder + GST + decode loop +
postnet; CBHG vocoder excluded) on BASELINE.json configs[1]: GST on, batch 32 per GPU, 128-token
utterances, Step_Reduction 2, Max_Step 1000, LJSpeech 80-mel hyper-parameters, fp32.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N>1 under a launcher: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...;
     N>1 WITHOUT a launcher: this process starts the N rank processes itself -- before anything touches the GPU -- and exits with
     their status.  A --gpus that disagrees with the launcher's WORLD_SIZE is an error, never a silent 1-rank run.)

A "step" is one Inference_Step over one synthetic batch per rank (inputs resident in HBM, weights
random-init of the reference architecture, randomness from the on-device Philox generator).
Utterances shard over ranks with no data-path collective; the only exchange is the final RCCL
gather of the mels to rank 0, which is inside the timed region.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, W warm-up steps, K timed steps, the line.  --full adds
what takes runs of its own: the per-kernel decode-step timings and the roofline (an event-bracketed graph, replayed
by the last timed step), the postnet alone, the bf16 drift against fp32 (--mixed), the several-batches-in-flight
figure and the CPU baseline.  --dump-outputs DIR writes what the last timed step returned (mel, stop, alignment) as
float32 .npy files; the inputs and seeds depend only on the arguments, so two builds can be compared file by file.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gst_tacotron_amd import distributed as gdist  # noqa: E402
from gst_tacotron_amd import synthetic, weights  # noqa: E402
from gst_tacotron_amd.model import GST_Tacotron  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MFMA_PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0}      # dense MFMA peaks (same guide; fp32-input MFMA = 1/16 of bf16)
# What a LONG MFMA loop sustains on real data (operands from LDS, every SIMD issuing back to back, the clock as the chip holds it: fp32 2.0-2.36 GHz;
# tools/msplit_bench.hip <rows> 100, tools/mfma_rate.hip, profiles/r04_msplit.txt).  Reported beside `peak`, never in its place.  (A ~20 us launch
# reaches two thirds of it: start-up and a clock that has not ramped.)
MFMA_SUSTAINED_TFLOPS = {"f32": 132.0, "bf16": 1650.0}
BATCH_PER_GPU = 32
PROFILE_EVERY = 20             # bracket every 20th decode step's LSTM launches with HIP events
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: above this, a fixed seeded sample of utterance rows is written


def host_cpu_info():
    """CPU model string and core counts of this box (lscpu; /proc/cpuinfo as fallback) -- BASELINE.md section 3 asks for them next
    to every CPU number."""
    info = {"model": None, "logical_cpus": os.cpu_count(), "physical_cores": None, "sockets": None}
    try:
        import subprocess
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {}
        for ln in out.splitlines():
            if ":" in ln:
                k, v = ln.split(":", 1)
                kv[k.strip()] = v.strip()
        info["model"] = kv.get("Model name")
        if "Socket(s)" in kv and "Core(s) per socket" in kv:
            info["sockets"] = int(kv["Socket(s)"])
            info["physical_cores"] = int(kv["Socket(s)"]) * int(kv["Core(s) per socket"])
    except Exception:
        pass
    if info["model"] is None:
        try:
            for ln in open("/proc/cpuinfo"):
                if ln.startswith("model name"):
                    info["model"] = ln.split(":", 1)[1].strip()
                    break
        except OSError:
            pass
    return info


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def cpu_baseline(hp, w, inputs, budget_s=15.0, runs=5):
    """The torch-CPU restatement of the TF2 graph (oracle/torch_ref.py, kind "port"; TensorFlow is not installable here)
    timed on this box's host cores, BASELINE.md section 3 protocol: 1 warm-up + `runs` timed runs, median (and min) reported,
    CPU model and thread count stated.  Two workloads:
      * like-for-like (the `value`): the bench's own configs[1] batch -- encoder + GST once, a BOUNDED number of decode
        steps, postnet on the frames those steps emit -- sized so that the timed runs take about `budget_s` seconds;
      * BASELINE configs[0], the reference's own CPU case, in full: GST off, batch 1, 32 tokens, Max_Step 200, r = 1.
    The protocol runs at 16, 32, 64 and all physical cores (up to 128) threads; `value` is the best median (eager per-op dispatch
    does not scale to every core), every count is reported under `by_threads`."""
    from oracle.torch_ref import TorchReference
    B, Tv = inputs["tokens"].shape
    d_r = int(hp["Step_Reduction"])
    total_steps = int(hp["Max_Step"]) // d_r
    rng = np.random.default_rng(123)
    masks, noise = synthetic.make_randomness(rng, total_steps, B, Tv, hp["Tacotron2"]["Decoder"]["Prenet"]["Size"])
    hp32 = dict(hp)
    hp32["Use_Mixed_Precision"] = False
    ref = TorchReference(hp32, w, torch.float32)

    def run(steps):
        t0 = time.perf_counter()
        ref.inference_step(inputs["tokens"], inputs.get("mels_for_gst"), inputs.get("mel_lengths_for_gst"),
                           masks[:steps], noise[:steps], steps=steps)
        return time.perf_counter() - t0

    cpu = host_cpu_info()
    ncpu = os.cpu_count() or 1
    # The whole protocol at BOTH candidate thread counts (eager per-op dispatch does not scale to every core, and which of
    # 16 / 32 wins differs from box to box and from run to run: a single calibration used to move the quoted GPU / CPU ratio by
    # 1.5x).  `value` is the better median; both are reported.
    per_thread = {}
    raw_times = {}
    best_step = None
    phys = cpu["physical_cores"] or ncpu
    for nt in sorted({min(ncpu, n) for n in (16, 32, 64, min(128, phys))}):
        torch.set_num_threads(nt)
        run(1)
        t1 = min(run(1), run(1))
        if nt > 32:
            # BASELINE.md section 3 says "all physical cores": on record even where it loses.  Eager per-op dispatch gets slower,
            # not faster, on many threads, so these counts get a short probe first and the whole protocol only if they are in reach
            t3 = run(3)
            probe_step = max((t3 - t1) / 2.0, 1e-4)
            if best_step is not None and probe_step > 2.0 * best_step:
                per_thread[nt] = {"value": B * d_r / probe_step, "probe_only": True, "decode_steps": 3,
                                  "note": "2-step probe only: {:.1f} ms per decode step, more than 2x the best thread count".format(probe_step * 1e3)}
                continue
        t9 = min(run(9), run(9))
        per_step = max((t9 - t1) / 8.0, 1e-4)
        best_step = per_step if best_step is None else min(best_step, per_step)
        per_run = budget_s / (2 * runs)
        steps_sample = int(max(10, min(total_steps, (per_run - t1) / per_step)))
        run(steps_sample)                                                   # warm-up
        times = [run(steps_sample) for _ in range(runs)]
        frames = B * steps_sample * d_r
        raw_times[nt] = times
        per_thread[nt] = {"value": frames / _median(times), "value_best_run": frames / min(times), "decode_steps": steps_sample,
                          "run_seconds": [round(t, 3) for t in times]}
    nt = max(raw_times, key=lambda k: per_thread[k]["value"])
    steps_sample = per_thread[nt]["decode_steps"]
    times = raw_times[nt]                                                   # (unrounded: the headline equals by_threads[nt])
    frames = B * steps_sample * d_r
    med, mn = _median(times), min(times)

    # BASELINE configs[0] in full (Model.py:249-255 with Device=-1): GST off, batch 1, 32 tokens, Max_Step 200, r = 1
    hp0, in0 = synthetic.config_inputs("cfg1")
    w0 = weights.synthetic_weights(hp0, seed=0)
    ref0 = TorchReference(hp0, w0, torch.float32)
    steps0 = int(hp0["Max_Step"]) // int(hp0["Step_Reduction"])
    m0, n0 = synthetic.make_randomness(np.random.default_rng(5), steps0, 1, in0["tokens"].shape[1],
                                       hp0["Tacotron2"]["Decoder"]["Prenet"]["Size"])

    def run0():
        t0 = time.perf_counter()
        ref0.inference_step(in0["tokens"], None, None, m0, n0, steps=steps0)
        return time.perf_counter() - t0

    best0 = None
    for nt0 in sorted({min(ncpu, n) for n in (1, 4, 8, 16)}):
        torch.set_num_threads(nt0)
        run0()
        t = run0()
        if best0 is None or t < best0[1]:
            best0 = (nt0, t)
    torch.set_num_threads(best0[0])
    times0 = [run0() for _ in range(runs)]
    frames0 = steps0 * int(hp0["Step_Reduction"])
    torch.set_num_threads(nt)
    return {"value": frames / med, "unit": "mel-frames/s", "cores": nt, "kind": "port",
            "value_best_run": frames / mn, "runs": runs, "run_seconds": [round(t, 3) for t in times],
            "by_threads": {str(k): v for k, v in per_thread.items()},
            "cpu_model": cpu["model"], "host_logical_cpus": cpu["logical_cpus"], "host_physical_cores": cpu["physical_cores"],
            "sample": "configs[1] batch {} x {} tokens: encoder+GST once, {} of {} decode steps, postnet on those {} frames; "
                      "median of {} runs after 1 warm-up, {:.2f} s per run on {} threads (the best of 16 / 32 / 64 / all physical cores up to 128, all in by_threads) of {}; "
                      "torch-CPU eager restatement of the TF2 graph (TF not installable)".format(
                          B, Tv, steps_sample, total_steps, steps_sample * d_r, runs, med, nt, cpu["model"]),
            "configs0": {"value": frames0 / _median(times0), "value_best_run": frames0 / min(times0), "unit": "mel-frames/s",
                         "cores": best0[0], "runs": runs, "run_seconds": [round(t, 3) for t in times0],
                         "sample": "BASELINE configs[0] in full: GST off, batch 1, 32 tokens, Max_Step 200, Step_Reduction 1 "
                                   "({} decode steps), whole Inference_Step; median of {} runs after 1 warm-up on {} threads "
                                   "(fastest of 1/4/8/16)".format(steps0, runs, best0[0])}}


def survey_step_bytes(d, B, Tv, mixed):
    """SURVEY.md section 8(d), "ALGORITHMIC work per unit": bytes of ONE decode step = every decoder weight once (stored width: 4 bytes,
    2 under Use_Mixed_Precision for the GEMM operands) + the activation rows of the batch once in and once out.  Returns
    (total, weights, activations).  configs[1]: 57.88 MB + 3.2 MB = 61.1 MB."""
    P0, P1, A_ = d.prenet[0], d.prenet[1], d.att
    H1, H2 = d.dec_rnn[0], d.dec_rnn[1]
    n_out = d.mel * d.r + 1
    n_w = (d.mel * P0 + P0) + (P0 * P1 + P1) + (P1 * A_ + A_) + (A_ + 1) + ((P1 + A_ + H1) * 4 * H1 + 4 * H1) + ((H1 + H2) * 4 * H2 + 4 * H2) + \
          ((H2 + A_) * n_out + n_out)
    wb = 2 if mixed else 4
    weights = wb * n_w
    acts = B * (Tv * A_ * 4 + 2 * Tv * 4 + 2 * 4 * H1 * 4 + (n_out + Tv) * 4)
    return weights + acts, weights, acts


def persistent_compulsory_bytes(d, B, Tv, mixed, steps):
    """What a persistent decode launch MUST move per launch, whatever it keeps resident: every weight once, the processed memory once
    (it lives in LDS afterwards), and per step the exchanged activations -- [prenet | context], h1, h2: written once and read at least
    once, at the width they travel in (4 bytes; 2 as bf16 mirrors under mixed precision) --, the noise row read and the outputs
    written (mel frames + stop logit + alignment row)."""
    P1, A_ = d.prenet[1], d.att
    H1, H2 = d.dec_rnn[0], d.dec_rnn[1]
    weights = survey_step_bytes(d, B, Tv, mixed)[1]
    sb = 2 if mixed else 4
    per_step = B * ((P1 + A_ + H1 + H2) * sb * 2 + (d.mel * d.r + 1 + Tv) * 4 + Tv * 4)
    return weights + B * Tv * A_ * 4 + steps * per_step


def ideal_ms(d, B, Tv, Tref, mixed, steps):
    """SURVEY 8(d) "Ideal time": decode = steps x step bytes / 8 TB/s; postnet, encoder, value projection and GST at the dense MFMA peak
    of the compute dtype.  configs[1]: 3.8 + 1.8 + 0.3 = 5.9 ms."""
    sb = survey_step_bytes(d, B, Tv, mixed)[0]
    peak = MFMA_PEAK_TFLOPS["bf16" if mixed else "f32"] * 1e12
    cin, post = d.mel, 0
    for f, kk in zip(d.post_filters, d.post_kernels):
        post += 2 * B * steps * d.r * kk * cin * f
        cin = f
    enc = B * (2 * Tv * (3 * 5 * 512 * 512 + 2 * 768 * 1024) + 2 * Tv * 640 * d.att + 2 * 25e6)     # encoder, value projection, GST
    return 1e3 * (steps * sb / (HBM_PEAK_GBS * 1e9) + (post + enc) / peak)


def pmc_traffic(kernel_substr, cfg_tag):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc summary of THIS configuration
    (profiles/<round>_<cfg_tag>_hbm_pmc.json: FETCH_SIZE x2 + WRITE_SIZE, separate passes, tools/profile.sh); None when
    no summary of this configuration is present."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_%s_hbm_pmc.json" % cfg_tag))) if cfg_tag else []
    if not files:
        return None, None
    try:
        data = json.load(open(files[-1]))
        for name, v in data.items():
            if kernel_substr in name:
                return v["hbm_read_bytes_corrected"] + v["hbm_write_bytes"], os.path.basename(files[-1])
    except Exception:
        pass
    return None, None


def rocprof_avg_us(kernel_substr, cfg_tag):
    """Average duration of the kernel in the committed rocprofv3 --kernel-trace --stats summary of THIS configuration
    (tools/profile.sh), for cross-reference with the live HIP-event figure (which includes ~2.5 us of event-node
    overhead); None if absent."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_%s_kernel_stats.csv" % cfg_tag))) if cfg_tag else []
    if not files:
        return None, None
    try:
        for r in csv.DictReader(open(files[-1])):
            if kernel_substr in r["Name"]:
                return float(r["AverageNs"]) * 1e-3, os.path.basename(files[-1])
    except Exception:
        pass
    return None, None


def serving_throughput(hp, w, holder, tok, mels, lens, device_index, B, Tv, Tref1, streams=4, steps=12):
    """NOT the headline `value` (which keeps ONE batch in flight: one decode loop, as configs[1] says).  The single loop is
    latency-bound -- 500 dependent steps of four dependent launches -- so a server with several independent requests queued gets
    more out of the GPU by keeping several of these loops in flight: `streams` contexts (one weight replica and workspace each)
    on `streams` HIP streams, the same batch-32 workload on each, `steps` whole Inference_Steps round-robin, wall clock."""
    import torch
    from gst_tacotron_amd.model import GST_Tacotron
    model = holder.pop()                 # (the caller's only reference: every context must be gone before the one-call measurement below)
    max_step, dev = model.dims.max_step, model.device
    models = [model] + [GST_Tacotron(hyper_parameters=hp, device=device_index, max_batch=B, max_tokens=Tv, max_ref_frames=Tref1).Restore(weights=w)
                        for _ in range(streams - 1)]
    strs = [torch.cuda.Stream(device=dev) for _ in range(streams)]
    del model

    def run(n, seed0):
        for i in range(n):
            with torch.cuda.stream(strs[i % streams]):
                models[i % streams].Inference_Step(tok, None, None, mels, lens, seed=seed0 + i)
        torch.cuda.synchronize()

    run(2 * streams, 5000)                           # captures each context's graph, warms up
    t0 = time.perf_counter()
    run(steps, 6000)
    dt = time.perf_counter() - t0
    frames = B * max_step * steps
    several = {"value": frames / dt, "ms_per_step": 1e3 * dt / steps, "streams": streams, "contexts": streams, "steps": steps}
    # The other way to serve the same queue (round 5): the `streams` requests as ONE call of streams x B utterances -- one context, one
    # weight replica, the decode loop as ONE persistent launch that runs the batch as groups of 32 rows through the resident weights
    # (csrc/persist_decode.hip, group kernels).  Needs the other contexts gone: the persistent launch is taken by a sole context.
    del models[:]
    import gc
    gc.collect()
    big = None
    try:
        Bb = B * streams
        mb = GST_Tacotron(hyper_parameters=hp, device=device_index, max_batch=Bb, max_tokens=Tv, max_ref_frames=Tref1).Restore(weights=w)
        tokb, melb, lenb = tok.repeat(streams, 1), mels.repeat(streams, 1, 1), lens.repeat(streams)
        for i in range(2):
            mb.Inference_Step(tokb, None, None, melb, lenb, seed=7000 + i)
        mb.synchronize()
        n = max(2, steps // streams)
        t0 = time.perf_counter()
        for i in range(n):
            mb.Inference_Step(tokb, None, None, melb, lenb, seed=8000 + i)
        torch.cuda.synchronize()
        dtb = time.perf_counter() - t0
        big = {"value": Bb * max_step * n / dtb, "ms_per_call": 1e3 * dtb / n, "batch": Bb, "calls": n,
               "persistent_decode_launches": mb.decode_counters()[0]}
        del mb
        gc.collect()
    except Exception as e:                            # (capacity, a give-up: the several-contexts figure stands alone)
        big = {"error": str(e)[:200]}
    best = max(several["value"], big.get("value", 0.0))
    return {"value": best, "unit": "mel-frames/s", "several_contexts": several, "one_call_of_all_requests": big,
            "note": "NOT the headline (which keeps ONE batch of 32 in flight): {} independent batch-{} requests served either as {} contexts on {} streams "
                    "(a weight replica each, launch path) or as one call of {} utterances (one persistent launch, groups of 32 rows through one set of "
                    "resident weights); `value` is the better of the two".format(streams, B, streams, streams, B * streams)}


def dump_outputs(path, arrays, max_bytes=DUMP_MAX_BYTES):
    """``--dump-outputs``: each array as ``path/<name>.npy`` in float32.  Above ``max_bytes`` in all, every array keeps the same
    fraction of its rows (utterances), chosen by a fixed seed, so that the files stay comparable from run to run."""
    os.makedirs(path, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > max_bytes:
            keep = max(1, int(a.shape[0] * max_bytes / total))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
            print("bench.py: {}.npy holds {} of {} rows (seeded sample: the outputs exceed {} MB)".format(
                name, keep, host[name].shape[0], max_bytes >> 20), file=sys.stderr, flush=True)
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def finish_line(line, lib_message, fallback_taken, fallback_note):
    """Rank 0: the library's last message and whether a fallback was taken go on the line, which is printed."""
    line["library_message"] = lib_message
    line["fallback_taken"] = fallback_taken
    if fallback_note:
        line["fallback_note"] = fallback_note
    print(json.dumps(line), flush=True)


def dry_run(args, overlap):
    """``--dry-run``: the N-rank control flow of this file on CPU ranks -- the launcher environment (or the self-spawned ranks), a gloo
    process group, ``gdist.run_steps`` with the chosen gather ordering around a stand-in for ``Inference_Step`` (a tensor that carries
    its rank and step), the all-reduced give-up flag and the max-over-ranks clock -- and rank 0's line, flagged ``dry_run`` and
    carrying NO measurement.  What it checks itself: the gathered batch holds every rank's rows in rank order for the LAST step, and
    the order in which steps were enqueued and gathers claimed is the one the knob promises."""
    rank, local_rank, world = gdist.init_process_group(backend="gloo")
    B, frames, mel = 4, 6, 5
    log = []

    def one_step(i):
        log.append(("enqueue", i))
        out = torch.full((B, frames, mel), float(1000 * i + rank))

        class Claim:
            def __init__(self, pend):
                self.pend = pend

            def result(self):
                log.append(("claim", i))
                return self.pend.result()
        return Claim(gdist.gather_to_root(out, n_total=B * world, async_op=True))
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    last = gdist.run_steps(args.steps, one_step, overlap_gather=overlap, first=args.warmup)
    elapsed = time.perf_counter() - t0
    want = []
    for i in range(args.warmup, args.warmup + args.steps):
        if overlap:
            want += [("enqueue", i)] + ([("claim", i - 1)] if i > args.warmup else [])
        else:
            want += [("enqueue", i), ("claim", i)]
    if overlap:
        want.append(("claim", args.warmup + args.steps - 1))
    assert log == want, (log, want)
    if world > 1:
        flag = torch.tensor([1 if (args.inject_give_up and rank == world - 1) else 0], dtype=torch.int32)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        any_gave_up = bool(flag.item())
        t = torch.tensor([elapsed], dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    else:
        any_gave_up = bool(args.inject_give_up)
    if rank == 0:
        i_last = args.warmup + args.steps - 1
        assert tuple(last.shape) == (B * world, frames, mel)
        for r in range(world):
            assert bool((last[r * B:(r + 1) * B] == float(1000 * i_last + r)).all()), r
        print(json.dumps({"metric": "mel-frames/s", "value": None, "unit": "mel-frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "dry_run": True, "data": "none (CPU ranks, gloo, a stand-in for the model: control flow only)",
                          "config": {"parallelism": "utterance-sharded x{} + final gather".format(world),
                                     "gather": "overlapped" if overlap else "claimed before the next batch is enqueued"},
                          "order": [list(e) for e in log], "fallback_taken": any_gave_up}), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: per-kernel decode-step timings and "
                    "the roofline, the postnet alone, the bf16 drift (--mixed), the serving figure and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step returned (mel, stop, alignment) "
                    "as DIR/<name>.npy, float32; above 64 MB in all, a fixed seeded sample of utterance rows")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-serving", action="store_true", help="--full: skip the several-batches-in-flight measurement (N = 1 only)")
    ap.add_argument("--mixed", action="store_true", help="Use_Mixed_Precision: bf16 GEMM operands, fp32 accumulation (BASELINE "
                    "configs[4]); NOT the headline metric -- dtype is then reported as bf16")
    ap.add_argument("--batch-per-gpu", type=int, default=BATCH_PER_GPU, help="utterances per GPU (default 32 = the headline "
                    "configuration; BASELINE configs[4] uses 64 with --mixed).  Any other value is NOT the headline metric")
    ap.add_argument("--inject-give-up", action="store_true", help="test hook: make the first timed run's in-kernel hand-off give up "
                    "(gsttaco_debug_raise_handoff_error), to exercise the discard-and-repeat path; the line then carries fallback_taken")
    ap.add_argument("--overlap-gather", type=int, default=None, choices=(0, 1), help="N > 1: 1 = batch i's RCCL gather is claimed after batch i + 1 has "
                    "been enqueued (the collective runs beside the next batch's compute); 0 = claimed before (the next batch's persistent decode "
                    "launch can then never meet a resident receive kernel).  Default 0: nobody could measure N > 1 for this repo, so the default is "
                    "the form that is safe by construction (gst_tacotron_amd.distributed.run_steps)")
    ap.add_argument("--dry-run", action="store_true", help="CPU ranks, gloo, a stand-in for the model: exercises the launcher, the process group, the "
                    "step / gather ordering, the give-up all-reduce and the line's assembly without a GPU (tests/test_host.py); the line carries "
                    "dry_run: true and no measurement")
    ap.add_argument("--cpu-seconds", type=float, default=25.0, help="--full: wall-time budget of the bounded CPU-baseline sample (both thread counts)")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # no launcher: start the N rank processes ourselves.  This parent has not touched the GPU (importing torch does not
        # initialise HIP) and never will: it only waits for its children and forwards their status.
        raise SystemExit(gdist.spawn_local_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))

    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world != args.gpus:
        raise SystemExit("bench.py: --gpus {} but the launcher's WORLD_SIZE is {}: refusing to print a line that would "
                         "misreport n_gpus".format(args.gpus, env_world))
    overlap = bool(args.overlap_gather) if args.overlap_gather is not None else False
    if args.dry_run:
        return dry_run(args, overlap)
    if torch.cuda.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: the HIP kernels are the only compute path")
    rank, local_rank, world = gdist.init_process_group(device_index=int(os.environ.get("LOCAL_RANK", "0")))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP kernels are the only compute path")
    torch.cuda.set_device(local_rank)
    if world > 1:
        world = torch.distributed.get_world_size()          # what the collective library actually sees
        assert world == args.gpus, (world, args.gpus)

    hp, inputs = synthetic.config_inputs("cfg2", batch=args.batch_per_gpu, seed=1 + rank)
    hp["Use_Mixed_Precision"] = bool(args.mixed)
    w = weights.synthetic_weights(hp, seed=0)
    B, Tv = inputs["tokens"].shape
    Tref1 = inputs["mels_for_gst"].shape[1]
    model = GST_Tacotron(hyper_parameters=hp, device=local_rank, max_batch=B, max_tokens=Tv, max_ref_frames=Tref1)
    model.Restore(weights=w)
    lib, handle = model.ctx.lib, model.ctx.handle

    dev = model.device
    tok = torch.as_tensor(inputs["tokens"]).to(dev)
    mels = torch.as_tensor(inputs["mels_for_gst"]).to(dev)
    lens = torch.as_tensor(inputs["mel_lengths_for_gst"]).to(dev)
    n_total = B * world
    last_i = args.warmup + args.steps - 1
    kept = {}                                      # the last timed step's local stop / alignment (--dump-outputs)

    def one_step(i):
        # dropout / noise streams are indexed by the LOCAL utterance index: fold the rank into the seed so that shards
        # do not draw identical randomness
        mel, stop, _, align = model.Inference_Step(tok, None, None, mels, lens, seed=(1000 + i) * world + rank)
        if i == last_i:
            kept["stop"], kept["alignment"] = stop, align
        # the gather runs on RCCL's stream behind this batch's compute; its result is claimed one step later, so that the
        # next batch's kernels are enqueued behind this batch's COMPUTE, not behind its gather (N = 1: no collective at all)
        return gdist.gather_to_root(mel, n_total=n_total, async_op=True)

    # --full: two cached graphs, the plain one and one whose decode launches are bracketed by event-record nodes on every
    # PROFILE_EVERY-th step.  Only the LAST timed step replays the bracketed graph (each bracket costs ~2.5 us, 200 of
    # them ~2 % of a step), so the kernel timings come from inside the timed region at 1/K of that cost.  A plain run
    # replays the plain graph only.
    def set_prof(on):
        model.ctx.check(lib.gsttaco_set_profiling(handle, PROFILE_EVERY if on else 0))

    def timed_run():
        """Warm-up + the timed region; returns the elapsed seconds (the clock stops after every gather has completed)."""
        if args.full:
            set_prof(True)
            one_step(-1).result()                  # capture + first replay of the bracketed graph (untimed, extra)
            set_prof(False)
        for i in range(args.warmup):
            one_step(i).result()
        if args.warmup == 0:
            one_step(0).result()                   # the plain graph must exist before the clock starts
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()

        def timed_step(i):
            if args.full and i == last_i:
                set_prof(True)
            return one_step(i)
        # (gather ordering: gdist.run_steps -- N > 1 claims batch i's gather before batch i + 1 is enqueued unless --overlap-gather 1)
        last = gdist.run_steps(args.steps, timed_step, overlap_gather=overlap, first=args.warmup)
        torch.cuda.synchronize()                   # every gather has completed before the clock stops
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, last

    # An in-kernel hand-off that gave up (persistent decode / BiLSTM / fused LSTM launch without co-residency: e.g. another process on
    # the GPU) produced garbage at full speed: gsttaco_synchronize says so after the clock has stopped, and the context has switched to
    # its launch-per-step forms (same results, slower).  That run is DISCARDED and the measurement is repeated once on those forms; the
    # line then says so (`fallback_taken`, `library_message`) -- a slower honest number instead of none.  A give-up during warm-up
    # leaves the same trace (a "warning:" text) and is flagged the same way.  A second failure is fatal.
    fallback_note = None
    if args.inject_give_up:
        model.ctx.check(lib.gsttaco_debug_raise_handoff_error(handle, 1 << 16))
    elapsed, out = timed_run()
    gave_up = None
    try:
        model.synchronize()
    except Exception as e:                          # GstTacoError: a hand-off gave up inside the run just timed
        gave_up = str(e)
    any_gave_up = gave_up is not None
    if world > 1:                                   # (every rank repeats when any rank's run was invalid: the job's time is the slowest rank's)
        flag = torch.tensor([1 if any_gave_up else 0], dtype=torch.int32, device=dev)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
        any_gave_up = bool(flag.item())
    if any_gave_up:
        fallback_note = "first timed run discarded: " + (gave_up or "a hand-off gave up on another rank")
        elapsed, out = timed_run()
        model.synchronize()
    lib_message = model.last_message()
    fallback_taken = fallback_note is not None or "warning" in lib_message
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    line = None
    if rank == 0:
        assert out is not None and tuple(out.shape) == (n_total, model.dims.steps * model.dims.r, model.dims.mel)
        assert bool(torch.isfinite(out).all())
        if args.dump_outputs:
            # what rank 0's caller of the timed path received in the last timed step: the gathered mels, its own stop logits and alignments
            dump_outputs(args.dump_outputs, {"mel": out, "stop": kept["stop"], "alignment": kept["alignment"]})
        frames = n_total * model.dims.max_step * args.steps
        line = {
            "metric": "mel-frames/s", "value": frames / elapsed, "unit": "mel-frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16" if args.mixed else "f32", "data": "synthetic",
            # what the dtype's arithmetic runs on: since round 6 the fp32 path's Winograd-domain GEMMs (postnet, encoder) and tall plain GEMMs run on the
            # bf16 matrix pipe as split-bf16 x6 (three bf16 planes per fp32 operand, six plane products, fp32 accumulation: the fp32 MFMA
            # chain's accuracy -- tools/split_bf16.hip, profiles/r06_split_bf16.txt); everything else of the fp32 path on fp32 MFMA / VALU
            "arith": ("bf16 operands, fp32 accumulate (Use_Mixed_Precision)" if args.mixed else
                      "fp32; the decode step on fp32 MFMA / VALU; the tall GEMMs around it (five-tap Conv1D layers of the postnet and the encoder as Winograd, "
                      "BiLSTM input halves, Value projection) as split-bf16 x6 on the bf16 matrix pipe, fp32 accumulate"
                      if os.environ.get("GSTTACO_WINO_SPLIT", "1") != "0" else "fp32"),
            "config": {"workload": ("" if args.batch_per_gpu == BATCH_PER_GPU and not args.mixed else "NOT THE HEADLINE CONFIGURATION -- ") +
                                   "BASELINE configs[1]: GST on, batch {} per GPU, 128-token utterances, ".format(args.batch_per_gpu) +
                                   "Step_Reduction 2, Max_Step 1000, LJSpeech 80-mel hparams; whole Inference_Step "
                                   "(encoder+GST+decode+postnet, vocoder excluded)",
                       "global_batch": n_total, "tokens": Tv, "ref_frames": Tref1 - 1,
                       "parallelism": "utterance-sharded x{} + final RCCL gather".format(world),
                       "gather": ("none (one rank)" if world == 1 else "overlapped with the next batch's compute (--overlap-gather 1)" if overlap else
                                  "claimed before the next batch is enqueued (safe by construction: a persistent decode launch never meets a resident receive kernel)")},
        }
    if not args.full:
        if rank == 0:
            finish_line(line, lib_message, fallback_taken, fallback_note)
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return 0

    # --full from here on.
    # per-kernel timing of the decode step: HIP event-record nodes inside the replayed graph (on the stream the
    # kernels run on), every PROFILE_EVERY-th decode step of the last timed replay
    big = B > 32            # batches above 32 rows run the multi-chunk kernels (weights resident over the chunks)
    lx = "gt_lstm_x_mc_kernel" if big else "gt_lstm_x_kernel"
    pj = "gt_proj_mc_kernel" if big else "gt_proj_lean_kernel"
    k1, k2 = ("2", "4") if args.mixed else ("3", "8")
    KNAMES = {0: lx + "<8," + k1 + "> LSTM layer 1 (input half + gates)", 1: lx + "<8," + k2 + "> LSTM layer 2 (input half + gates)",
              2: "gt_dec_front_lean_kernel (prenet + query + attention per utterance; workers: recurrent halves W_h.h+b)",
              3: pj + " (projection + next prenet-0; workers: layer-2 recurrent half)"}
    KPMC = {0: lx + "<8, " + k1 + ", 1", 1: lx + "<8, " + k2 + ", 2", 2: "gt_dec_front_lean_kernel<8, 4, " + ("2" if args.mixed else "1"), 3: pj}
    prof = {}
    for which in range(4):
        ms, cnt = ctypes.c_float(), ctypes.c_int()
        model.ctx.check(lib.gsttaco_get_profile(handle, which, ctypes.byref(ms), ctypes.byref(cnt)))
        prof[which] = (ms.value, cnt.value, int(lib.gsttaco_lstm_launch_bytes(handle, which, B)))
    n_steps_dec = model.dims.steps
    _dc = model.decode_counters()
    persistent = _dc[0] > 0 and _dc[1] != 0        # (after a give-up the persistent form is off: the timed run was launches)
    if persistent:
        # the whole decode loop ran as ONE persistent launch (csrc/persist_decode.hip): one bracket around it; a decode step is
        # 1 / steps of it.  Algorithmic bytes per step EXACTLY as SURVEY 8(d) defines them (every weight once PER STEP + the activations:
        # 61.1 MB at configs[1]), although this kernel keeps the weights in registers: the compulsory variant (weights once per LAUNCH)
        # and the counted traffic are reported beside it.
        step_bytes_all, w_bytes, act_bytes = survey_step_bytes(model.dims, B, Tv, args.mixed)
        ms_total, cnt_total = prof[2][0], prof[2][1]
        prof = {2: (ms_total / n_steps_dec, cnt_total * n_steps_dec, step_bytes_all)}
        kname = "gt_persist_decode_h_kernel" if args.mixed else "gt_persist_decode_kernel" if B <= 32 else "gt_persist_decode_g_kernel"
        KNAMES[2] = (kname + ", 1 / {} of it (the whole decoder loop as ONE persistent launch: weights resident in registers, "
                     "processed memory in LDS, in-kernel hand-offs; a step = prenet + query + attention + both LSTM cells + projection".format(n_steps_dec) +
                     ("; bf16 operands, one group of up to 64 rows, activations as bf16 mirrors" if args.mixed else
                      "" if B <= 32 else "; {} groups of 32 rows through the resident weights".format((B + 31) // 32)) + ")")
        KPMC[2] = kname
    elif prof[1][1] == 0 and prof[0][1] > 0:
        # both decode LSTM cells ran as ONE launch (gt_lstm12_kernel, in-kernel hand-off of h1): one bracket, both cells' bytes
        prof[0] = (prof[0][0], prof[0][1], prof[0][2] + prof[1][2])
        del prof[1]
        KNAMES[0] = ("gt_lstm12_mc_kernel" if big else "gt_lstm12_kernel") + " (both LSTM cells: input halves + gates, h1 handed over in-kernel)"
        KPMC[0] = "gt_lstm12_mc_kernel" if big else "gt_lstm12_kernel"
    # An event-record node is a graph node of its own, so a bracketed kernel reads ~2-3 us longer than rocprofv3
    # --kernel-trace reports for it (profiles/*_kernel_stats.csv); the figures are NOT corrected (conservative: the
    # roofline fraction is understated).  The empty bracket (two event nodes back to back) is reported for reference.
    ms, cnt = ctypes.c_float(), ctypes.c_int()
    model.ctx.check(lib.gsttaco_get_profile(handle, 4, ctypes.byref(ms), ctypes.byref(cnt)))
    bracket_ms = ms.value

    # the postnet alone (its own C-ABI entry point on this stream), timed with events after the clock has stopped: its
    # direct-equivalent FLOP rate against the MFMA peak of the precision it runs in
    post = None
    if rank == 0:
        d = model.dims
        pre = torch.randn((B, d.steps * d.r, d.mel), device=dev).clamp_(-4, 4)
        model.postnet(pre)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            model.postnet(pre)
        e1.record()
        torch.cuda.synchronize()
        post_ms = e0.elapsed_time(e1) / 5
        cin, fl = d.mel, 0
        for f, kk in zip(d.post_filters, d.post_kernels):           # Taco2.py:131-149
            fl += 2 * B * d.steps * d.r * kk * cin * f
            cin = f
        peak = MFMA_PEAK_TFLOPS["bf16" if args.mixed else "f32"]
        # FLOP the kernels actually ISSUE: Winograd F(4,5) does 8 transform-domain GEMMs per 4 output frames (0.4x the direct
        # form's multiplications), F(2,5) 6 per 2 (0.6x); fp32 only -- the bf16 path is the direct form.  (Which layers take which:
        # gemm_conv.hip gt_launch_conv_gemm -- five taps, Cin and Cout multiples of 4; F(4,5) where its grid fills the chip.)
        fl_issued, cin, Tf = 0.0, d.mel, d.steps * d.r
        for f, kk in zip(d.post_filters, d.post_kernels):
            lf = 2.0 * B * Tf * kk * cin * f
            if not args.mixed and kk == 5 and cin % 4 == 0 and f % 4 == 0:
                nb, cpad = -(-f // 128), max(128, -(-cin // 64) * 64)           # (padded input channels are multiplied too)
                if -(-(B * -(-Tf // 4)) // 64) * nb >= 240:
                    lf *= 0.4 * cpad / cin
                elif -(-(B * -(-Tf // 2)) // 64) * nb >= 240:
                    lf *= 0.6 * cpad / cin
            fl_issued += lf
            cin = f
        split = (not args.mixed) and os.environ.get("GSTTACO_WINO_SPLIT", "1") != "0"
        if split:
            # (round 6) the Winograd-domain GEMMs run on the bf16 pipe as split-bf16 x6: SIX bf16 multiply-adds per fp32-equivalent one
            # are issued, and the fraction is priced against the pipe they run on
            post = {"ms": post_ms, "direct_equivalent_flop": fl, "TFLOP/s": fl / (post_ms * 1e-3) / 1e12,
                    "arith": "Winograd F(4,5)/F(2,5), transform-domain GEMMs as split-bf16 x6 (three bf16 planes per fp32 operand, products hh hm mh mm hl lh, fp32 accumulate)",
                    "peak_TFLOP/s": MFMA_PEAK_TFLOPS["bf16"], "issued_flop": 6.0 * fl_issued,
                    "frac": 6.0 * fl_issued / (post_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS["bf16"],
                    "fp32_equivalent_issued_flop": fl_issued,
                    "frac_fp32_equivalent": fl_issued / (post_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS["f32"],
                    "frac_direct_equivalent": fl / (post_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS["f32"],
                    "note": "`frac` = bf16 FLOP the kernels ISSUE (6 per Winograd-domain fp32 multiply-add) / time / the dense bf16 MFMA peak; "
                            "`frac_fp32_equivalent` = the Winograd-domain fp32 FLOP / time / the fp32 MFMA peak (the pipe the round-5 kernel ran on: "
                            "0.52-0.55 there); `frac_direct_equivalent` the direct form's (can exceed 1)"}
        else:
            post = {"ms": post_ms, "direct_equivalent_flop": fl, "TFLOP/s": fl / (post_ms * 1e-3) / 1e12, "peak_TFLOP/s": peak,
                    "frac_direct_equivalent": fl / (post_ms * 1e-3) / 1e12 / peak,
                    "issued_flop": fl_issued, "frac": fl_issued / (post_ms * 1e-3) / 1e12 / peak,
                    "note": "5 Conv1D(k=5) layers as Winograd F(4,5)/F(2,5) (0.4x / 0.6x the multiplications of the direct form) in fp32, "
                            "direct-form GEMM on bf16 MFMA under --mixed; `frac` counts the FLOP the kernels ISSUE (Winograd-domain GEMMs), "
                            "`frac_direct_equivalent` the direct form's (can exceed 1 for a Winograd kernel)"}

    if rank == 0:
        dom = max(prof, key=lambda k: prof[k][0])          # dominant = largest share of the decode step
        ms1, cnt1, bytes1 = prof[dom]
        achieved_in_run = (bytes1 / (ms1 * 1e-3)) / 1e9 if ms1 > 0 else 0.0
        # which committed profile belongs to this run: BASELINE configs[1] (the headline), the configs[2]-sized batch, the configs[4] shard
        cfg_tag = {(32, False): "cfg2", (128, False): "cfg3", (64, True): "cfg5"}.get((args.batch_per_gpu, bool(args.mixed)))
        traffic, traffic_src = pmc_traffic(KPMC[dom], cfg_tag)
        rp_us, rp_src = rocprof_avg_us(KPMC[dom], cfg_tag)
        if persistent:          # (the committed figures are per launch = per decode loop; everything below is per step)
            rp_us = rp_us / n_steps_dec if rp_us else None
            traffic = traffic / n_steps_dec if traffic else None
        step_us = sum(v[0] for v in prof.values()) * 1e3
        step_bytes = sum(v[2] for v in prof.values())
        # the decode step's GEMM work (prenet-1, query, both LSTM cells, projection + fused prenet-0): what bounds it at batches
        # above 32 rows, where fp32 MFMA time overtakes the weight stream
        dd = model.dims
        P0, P1, A_ = dd.prenet[0], dd.prenet[1], dd.att
        H1, H2 = dd.dec_rnn[0], dd.dec_rnn[1]
        step_flop = 2 * B * (P0 * P1 + P1 * A_ + (P1 + A_ + H1) * 4 * H1 + (H1 + H2) * 4 * H2 + (H2 + A_) * (dd.mel * dd.r + 1 + P0))
        mfma_peak = MFMA_PEAK_TFLOPS["bf16" if args.mixed else "f32"]
        step_frac_hbm = (step_bytes / step_us / 1e3) / HBM_PEAK_GBS if step_us > 0 else 0.0
        step_frac_mfma = (step_flop / (step_us * 1e-6) / 1e12) / mfma_peak if step_us > 0 else 0.0
        step_bound = "mfma" if step_frac_mfma > step_frac_hbm else "hbm"
        # The dominant launch against the roofline that bounds the step.  Its duration: the committed rocprofv3 --kernel-trace
        # average of THIS configuration when one exists (what profiles/ reproduces), else the in-run bracket minus the measured
        # empty bracket; the raw in-run figure (an event node is a graph node of its own: it reads 2.5-3.5 us long) stays beside it.
        # A persistent launch is bracketed ONCE for all of its steps (the ~3 us an event node costs vanish in 10 ms): its duration is the one
        # measured live in this run, and the committed rocprofv3 average is the cross-check beside it (avg_launch_us_rocprofv3).
        dur_us = ms1 * 1e3 if persistent else (rp_us if rp_us else max(ms1 * 1e3 - bracket_ms * 1e3, 1e-3))
        # the dominant launch's own GEMM work: its share of the step's FLOP by its share of the step's algorithmic bytes is wrong
        # for the front launch (weights of two layers' recurrent halves); count it from the launch's GEMMs instead
        launch_flop = {0: 2 * B * ((P1 + A_) * 4 * H1 + H1 * 4 * H2) if 1 not in prof else 2 * B * (P1 + A_) * 4 * H1,
                       1: 2 * B * H1 * 4 * H2,
                       2: 2 * B * (P0 * P1 + P1 * A_) + 2 * B * H1 * 4 * H1 + 2 * B * H2 * 4 * H2 * (1.0 - (128.0 if B > 32 else 64.0) / max(H2 // 4, 1)),
                       3: 2 * B * (H2 + A_) * (dd.mel * dd.r + 1 + P0) + 2 * B * H2 * 4 * H2 * ((128.0 if B > 32 else 64.0) / max(H2 // 4, 1))}[dom]
        if persistent:
            launch_flop = step_flop
        if step_bound == "mfma":
            achieved, peak, unit = launch_flop / (dur_us * 1e-6) / 1e12, mfma_peak, "TFLOP/s"
            achieved_raw = launch_flop / (ms1 * 1e-3) / 1e12 if ms1 > 0 else 0.0
        else:
            achieved, peak, unit = bytes1 / (dur_us * 1e-6) / 1e9, HBM_PEAK_GBS, "GB/s"
            achieved_raw = achieved_in_run
        line.update({
            "roofline": {"bound": step_bound, "kernel": KNAMES[dom],
                         "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak,
                         "frac_basis": ("measured live in this run: HIP event-record nodes inside the replayed graph around the ONE persistent launch of the last timed "
                                        "step, / its steps; avg_launch_us_rocprofv3 is the committed rocprofv3 --kernel-trace average of this configuration "
                                        "(another box) for cross-reference" if persistent else
                                        ("the committed rocprofv3 --kernel-trace average of this configuration (rocprofv3_source)" if rp_us else
                                         "in-run HIP event-record nodes around the launch minus the measured empty bracket") +
                                        "; frac_in_run divides by the raw in-run bracket (an event node is a graph node of its own: understated)"),
                         "frac_in_run": achieved_raw / peak,
                         "frac_hbm_rocprofv3": (bytes1 / (rp_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if rp_us else None,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_note": "FETCH_SIZE x2 + WRITE_SIZE per launch from the COMMITTED rocprofv3 --pmc profile named in "
                                         "traffic_source (separate passes, tools/profile.sh); a constant, not measured in this run",
                         "served_from": "weights: Infinity Cache (the 58 MB per-step working set is re-read every step and stays "
                                        "resident in the 256 MiB MALL; the memory-side counters count those hits); shared "
                                        "activations: XCD L2.  `peak` is the HBM3E spec rate the guide names for the hbm bound",
                         "bytes_per_launch": bytes1 * (n_steps_dec if persistent else 1),
                         "bytes_per_step": bytes1,
                         "bytes_basis": ("SURVEY.md section 8(d): every decoder weight once per decode step at its stored width + the batch's activation "
                                         "rows once in and once out" + (" ({:.2f} MB per step x {} steps per launch)".format(bytes1 / 1e6, n_steps_dec) if persistent else "")),
                         "end_to_end_frac": ideal_ms(model.dims, B, Tv, Tref1 - 1, args.mixed, n_steps_dec) / (1e3 * elapsed / args.steps),
                         "end_to_end_ideal_ms": ideal_ms(model.dims, B, Tv, Tref1 - 1, args.mixed, n_steps_dec),
                         "bound_effective": "latency" if persistent else step_bound,
                         "limiter": ("dependent hand-offs and one CU's per-utterance chain (latency), not bytes: this launch keeps its weights in registers, "
                                     "so `frac` (algorithmic bytes, the contract's definition) overstates what the memory system does -- see "
                                     "persistent_decode.frac_compulsory and frac_traffic" if persistent else None),
                         "frac_traffic": (traffic / (dur_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if (traffic and dur_us) else None,
                         "persistent_decode": ({"launch_us": ms1 * 1e3 * n_steps_dec, "steps_per_launch": n_steps_dec,
                                                "compulsory_bytes_per_step": persistent_compulsory_bytes(model.dims, B, Tv, args.mixed, n_steps_dec) / n_steps_dec,
                                                "frac_compulsory": persistent_compulsory_bytes(model.dims, B, Tv, args.mixed, n_steps_dec) / n_steps_dec /
                                                                   (dur_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                                "note": "achieved / frac price the step at SURVEY 8(d)'s algorithmic bytes (every weight once per step); "
                                                        "this kernel reads the weights once per LAUNCH -- frac_compulsory counts them so, frac_traffic is "
                                                        "what the counters saw (polling included): the step is bound by its dependent hand-offs "
                                                        "(in-kernel all-to-alls of h1 / h2, ~2.4 us each) and the per-utterance chain, not by bytes"}
                                               if persistent else None),
                         "avg_launch_us": ms1 * 1e3, "launches_timed": cnt1, "empty_event_bracket_us": bracket_ms * 1e3,
                         "avg_launch_us_rocprofv3": rp_us, "rocprofv3_source": rp_src,
                         "step_frac": max(step_frac_hbm, step_frac_mfma),
                         "step_bound": step_bound,
                         "step_frac_note": "whole decode step (one persistent launch for all steps, or 3-4 launches per step; x 500 = 86 % of the run): algorithmic bytes / sum of the bracketed "
                                           "launch times / 8 TB/s, or GEMM FLOP / the same time / the dense MFMA peak of the compute "
                                           "dtype, whichever is larger (fp32 MFMA overtakes the weight stream above 32 rows)",
                         "mfma_sustained": {"TFLOP/s": MFMA_SUSTAINED_TFLOPS["bf16" if args.mixed else "f32"],
                                            "source": "profiles/r04_msplit.txt (tools/msplit_bench.hip, tools/mfma_rate.hip): a long MFMA loop of the compute dtype on "
                                                      "random operands, clock as the chip holds it; `peak` and every `frac` use the guide's figure"},
                         "postnet": post,
                         "decode_step": {"us": step_us, "algorithmic_bytes": step_bytes,
                                         "GB/s": step_bytes / step_us / 1e3 if step_us > 0 else 0.0,
                                         "frac_hbm": step_frac_hbm, "gemm_flop": step_flop,
                                         "TFLOP/s": step_flop / (step_us * 1e-6) / 1e12 if step_us > 0 else 0.0, "frac_mfma": step_frac_mfma,
                                         "kernels": {str(k): dict({"name": KNAMES[k], "avg_us": prof[k][0] * 1e3, "bytes": prof[k][2]},
                                                                  **({"algorithmic_bytes_per_launch": prof[k][2] * n_steps_dec,
                                                                      "compulsory_bytes_per_launch": persistent_compulsory_bytes(model.dims, B, Tv, args.mixed, n_steps_dec)}
                                                                     if persistent else {}))
                                                     for k in prof}}},
        })
        if args.mixed:
            # what the mode costs in accuracy, MEASURED on this run's inputs: the same batch, weights and seed (same keep decisions and noise)
            # through an fp32 context; mel max-abs / mean-abs difference after the postnet, on the +-4 mel range.  (BASELINE configs[4]'s
            # bar "mel max-abs <= 1e-3" is the fp32 bar; the mode's own tolerances are tests/test_gpu_parity.py MIXED_TOL / MIXED_MEAN.)
            try:
                hp32 = dict(hp); hp32["Use_Mixed_Precision"] = False
                m32 = GST_Tacotron(hyper_parameters=hp32, device=local_rank, max_batch=B, max_tokens=Tv, max_ref_frames=Tref1)
                m32.Restore(weights=w)
                a16 = model.Inference_Step(tok, None, None, mels, lens, seed=4242)[0]
                a32 = m32.Inference_Step(tok, None, None, mels, lens, seed=4242)[0]
                torch.cuda.synchronize()
                dmel = (a16 - a32).abs()
                line["mixed_drift"] = {"mel_max_abs_vs_fp32": float(dmel.max()), "mel_mean_abs_vs_fp32": float(dmel.mean()),
                                       "frames": int(a16.shape[1]), "note": "bf16-operand path against the fp32 path of this library on the same batch, "
                                       "weights, keep decisions and noise; the trajectories separate over 500 autoregressive steps (a flipped bf16 "
                                       "rounding is fed back), so the max is a property of the synthetic model as much as of the arithmetic"}
                del m32
            except Exception as e:
                line["mixed_drift"] = {"error": str(e)[:200]}
        if world == 1 and not args.no_serving:
            holder = [model]
            del model                    # (the closures above are done; the serving measurement needs to be able to drop the last context)
            line["serving"] = serving_throughput(hp, w, holder, tok, mels, lens, local_rank, B, Tv, Tref1)
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(hp, w, inputs, args.cpu_seconds)
        finish_line(line, lib_message, fallback_taken, fallback_note)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
