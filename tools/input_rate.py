"""Cost of turning one RGB batch (32 images of 300x300) into the model's DCT input tensors, host path vs device path:

  (a) host:   data/jpeg_dct.py:emit_dct_inputs (PIL encode, in-tree entropy decoder on 16 threads) + float32 upload
  (b) device: uint8 upload + dj_rgb_to_dct
  (c) the kernel alone, by device events, and its bytes moved over that time
  (d) Model.fit_generator img/s on the deconv SSD300 workload, fed by a generator that emits the same prepared pixel
      batches through (a) or through DeviceDCTEmitter (labels through DeviceLabelEncoder both times)

    python tools/input_rate.py [--reps 30] [--fit-steps 60] [--no-fit]

Medians over `reps` after warm-up; every timed window ends in a device synchronise.  (a) and the host half of (d) need
PIL; without it they are reported as not measured.  Prints one JSON line at the end."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import kernels, workloads
from jpeg_detection_resnet_ssd_amd.data import jpeg_dct
from jpeg_detection_resnet_ssd_amd.data import synthetic_dct as sd

HBM_MEASURED_GBS = 6290.0     # float4 copy on MI355X


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fit-steps", type=int, default=60)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "input_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    B = 32
    rng = np.random.default_rng(0)
    batches = [np.stack([sd.smooth_random_image(rng) for _ in range(B)]) for _ in range(2)]
    pixels = batches[0]
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    res = {"batch": B, "image": [300, 300], "reps": args.reps, "pil": have_pil}
    shapes = jpeg_dct.input_shapes(B, 300, 300, deconv=True)
    bufs = [torch.empty(s, device=dev) for s in shapes]
    tabs = jpeg_dct.quant_tables(75)

    # (a) host path
    if have_pil:
        def host_path():
            for buf, arr in zip(bufs, jpeg_dct.emit_dct_inputs(pixels, deconv=True, n_threads=16)):
                buf.copy_(torch.from_numpy(arr), non_blocking=True)
        res["host_ms"] = median_ms(host_path, max(5, args.reps // 3))
        want = [b.clone() for b in bufs]
    # (b) device path
    def device_path():
        d = torch.from_numpy(pixels).to(dev, non_blocking=True)
        kernels.rgb_to_dct(d, tabs, tuple(bufs))
    res["device_ms"] = median_ms(device_path, args.reps)
    if have_pil:
        res["device_equals_host"] = all(torch.equal(a, b) for a, b in zip(want, bufs))
        res["host_over_device"] = res["host_ms"][0] / res["device_ms"][0]
    # uint8 upload alone (what the kernel must stay below)
    res["upload_u8_ms"] = median_ms(lambda: torch.from_numpy(pixels).to(dev, non_blocking=True), args.reps)
    pinned = torch.from_numpy(pixels).pin_memory()
    res["upload_u8_pinned_ms"] = median_ms(lambda: pinned.to(dev, non_blocking=True), args.reps)
    # (c) kernel alone, by events
    d = torch.from_numpy(pixels).to(dev)
    for _ in range(5):
        kernels.rgb_to_dct(d, tabs, tuple(bufs))
    times = []
    for _ in range(max(50, args.reps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels.rgb_to_dct(d, tabs, tuple(bufs))
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    k_ms = statistics.median(times)
    moved = pixels.nbytes + sum(4 * int(np.prod(s)) for s in shapes)
    res["kernel_ms"] = (k_ms, min(times), max(times))
    res["kernel_bytes"] = moved
    res["kernel_GBs"] = moved / k_ms / 1e6
    res["kernel_share_of_measured_hbm"] = res["kernel_GBs"] / HBM_MEASURED_GBS
    res["kernel_below_u8_upload"] = k_ms < res["upload_u8_pinned_ms"][0]
    print(json.dumps(res), flush=True)

    # (d) fit_generator
    if not args.no_fit:
        from jpeg_detection_resnet_ssd_amd.ssd_encoder_decoder.ssd_input_encoder import DeviceLabelEncoder
        model, sizes = workloads.build_ssd("deconv")
        enc = DeviceLabelEncoder(workloads.make_encoder(sizes))
        gts = [sd.random_ground_truth(B, seed=i) for i in range(len(batches))]
        emitter = jpeg_dct.DeviceDCTEmitter(quality=75, deconv=True)

        def gen(device_side):
            for i in itertools.cycle(range(len(batches))):
                x = emitter(batches[i]) if device_side else jpeg_dct.emit_dct_inputs(batches[i], deconv=True, n_threads=16)
                yield x, enc(gts[i])
        order = [True, False, True, False] if have_pil else [True, True]
        rates = {True: [], False: []}
        for device_side in order:
            g = gen(device_side)
            model.fit_generator(g, steps_per_epoch=5, epochs=1, verbose=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.fit_generator(g, steps_per_epoch=args.fit_steps, epochs=1, verbose=0)
            torch.cuda.synchronize()
            rates[device_side].append(B * args.fit_steps / (time.perf_counter() - t0))
        res["fit_img_s_device_dct"] = rates[True]
        res["fit_img_s_host_dct"] = rates[False] if have_pil else "not measured (no PIL)"
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
