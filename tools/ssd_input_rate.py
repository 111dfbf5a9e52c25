"""Cost of turning one batch of decoded images (32 images of mixed sizes around 375x500) into the SSD300 DCT input tensors
through the geometric stages of `SSDDataAugmentation` (expand, random crop, flip, resize to 300x300), host path vs device
path, with the geometries drawn by `SSDDataAugmentation.plan` under a fixed seed:

  (a) host:   the chain in pixel mode on 16 threads (numpy canvas, Pillow resize), data/jpeg_dct.py:emit_dct_inputs (PIL
              encode, in-tree entropy decoder on 16 threads), float32 upload
  (b) device: `plan` per image, DevicePatchResize: one upload of descriptors + taps + the covered rectangles from pinned
              memory, dj_patch_resize, dj_rgb_to_dct
  (c) the two kernels alone, by device events, and their bytes moved over that time; the pinned upload of their input
  (d) the photometric stage (`SSDPhotometricDistortions`, drawn per image under the same seed, before the geometry, as the
      chain draws it): the host statement `ssd_photometric_host` on 16 threads (`photometric_host_ms`), the device path
      with the stage (`device_photometric_ms` beside `device_ms`, `device_photometric_emit_only_ms` beside
      `device_emit_only_ms`), and dj_ssd_photometric alone by events on the staged rectangles (`ssd_photometric_ms`, bytes
      read and written once each) beside `patch_resize_ms` on the same batch

    python tools/ssd_input_rate.py [--reps 20]

`device_ms` contains the draws and the box arithmetic of `plan` (`chain_plan_ms`, host numpy that both paths need);
`host_ms` starts from the planned geometries and does not, so the stage-for-stage comparison is `host_ms` against
`device_emit_only_ms` + `patch_plan_ms`.

Medians over `reps` after warm-up; every timed window ends in a device synchronise.  The host path resizes with
`Image.resize` on the planned window (what `patch_resize_host` states in numpy, at Pillow's speed), so (a) and (b) are
compared on bit-identical tensors (`device_equals_host`).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import kernels
from jpeg_detection_resnet_ssd_amd.data import jpeg_dct, patch_resize, ssd_augment

HBM_MEASURED_GBS = 6290.0     # float4 copy on MI355X (tools/input_rate.py)
OUT = 300


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


def event_ms(fn, reps):
    for _ in range(5):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def make_batch(rng, n):
    """Smooth content plus noise, landscape and portrait, sides within +-15 % of 375 x 500, two to four boxes each."""
    images, labels = [], []
    for i in range(n):
        h, w = int(375 * rng.uniform(0.85, 1.15)), int(500 * rng.uniform(0.85, 1.15))
        if i % 3 == 2:
            h, w = w, h
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / (11.0 + c + i % 7) + c) * np.cos(yy / (8.0 + 2 * c)) for c in range(3)], axis=-1)
        images.append(np.clip(img + rng.normal(0, 15, img.shape), 0, 255).astype(np.uint8))
        rows = []
        for _ in range(int(rng.integers(2, 5))):
            bw, bh = int(rng.integers(40, w // 2)), int(rng.integers(40, h // 2))
            x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            rows.append([int(rng.integers(1, 21)), x0, y0, x0 + bw, y0 + bh])
        labels.append(np.array(rows))
    return images, labels


def pil_patch(image, geometry):
    from PIL import Image
    return np.asarray(Image.fromarray(ssd_augment.window_host(image, geometry)).resize((OUT, OUT), geometry[5]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ssd_input_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    B = 32
    images, labels = make_batch(np.random.default_rng(0), B)
    chain = ssd_augment.SSDDataAugmentation(OUT, OUT)

    def plan_all():
        np.random.seed(1)
        return [chain.plan(im.shape[0], im.shape[1], y)[0] for im, y in zip(images, labels)]
    geometries = plan_all()
    import PIL
    res = {"batch": B, "out": OUT, "reps": args.reps, "pil": PIL.__version__, "source_MB": sum(im.nbytes for im in images) / 1e6,
           "expanded": sum(g[2] > im.shape[0] for g, im in zip(geometries, images)), "flipped": sum(bool(g[4]) for g in geometries),
           "filters": [int(g[5]) for g in geometries]}
    shapes = jpeg_dct.input_shapes(B, OUT, OUT, deconv=True)
    bufs = [torch.empty(s, device=dev) for s in shapes]
    pool = ThreadPoolExecutor(16)

    # (a) host path: the planned windows cut and resized on 16 threads, then the JPEG round trip and the upload
    def host_pixels():
        return np.stack(list(pool.map(lambda a: pil_patch(*a), zip(images, geometries))))

    def host_path():
        for buf, arr in zip(bufs, jpeg_dct.emit_dct_inputs(host_pixels(), deconv=True, n_threads=16)):
            buf.copy_(torch.from_numpy(arr), non_blocking=True)
    res["host_ms"] = median_ms(host_path, max(5, args.reps // 2))
    res["host_window_resize_ms"] = median_ms(host_pixels, max(5, args.reps // 2))
    want = [b.clone() for b in bufs]
    # (b) device path: plan, descriptors and taps, staging, one upload, the two kernels
    prep = patch_resize.DevicePatchResize(OUT, OUT, deconv=True)
    res["device_ms"] = median_ms(lambda: prep(images, plan_all()).emit_into(bufs), args.reps)
    res["device_equals_host"] = all(torch.equal(a, b) for a, b in zip(want, bufs))
    res["host_over_device"] = res["host_ms"][0] / res["device_ms"][0]
    pending = prep(images, geometries)
    res["device_emit_only_ms"] = median_ms(lambda: pending.emit_into(bufs), args.reps)
    res["chain_plan_ms"] = median_ms(plan_all, args.reps)
    res["patch_plan_ms"] = median_ms(lambda: prep(images, geometries), args.reps)
    # (c) the two kernels alone, by events, beside the upload of their input
    plan = pending.plan
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    plan.fill(staging.numpy(), images)
    res["upload_pinned_ms"] = median_ms(lambda: staging.to(dev, non_blocking=True), args.reps)
    res["upload_MB"], res["staged_share_of_source"] = plan.nbytes / 1e6, plan.src_bytes / sum(im.nbytes for im in images)
    blob = staging.to(dev)
    pixels = torch.empty((B, OUT, OUT, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    host = staging.numpy()
    reps = max(50, args.reps)
    patch_ms = event_ms(lambda: plan.launch(host, blob, pixels, scratch), reps)
    outs = tuple(bufs)
    dct_ms = event_ms(lambda: kernels.rgb_to_dct(pixels, prep.tables, outs), reps)
    d = plan.desc
    rows = d["win_h"].astype(np.int64)
    # staged rectangles read once, the scratch written and read, the output written, the pool read
    patch_bytes = int((d["src_h"].astype(np.int64) * d["src_stride"]).sum() + 2 * (rows * 3 * OUT).sum() + B * OUT * OUT * 3
                      + plan.pool.nbytes)
    dct_bytes = B * OUT * OUT * 3 + sum(4 * int(np.prod(s)) for s in shapes)
    res["patch_resize_ms"], res["patch_resize_bytes"] = patch_ms, patch_bytes
    res["patch_resize_GBs"] = patch_bytes / patch_ms[0] / 1e6
    res["rgb_to_dct_ms"], res["rgb_to_dct_bytes"], res["rgb_to_dct_GBs"] = dct_ms, dct_bytes, dct_bytes / dct_ms[0] / 1e6
    res["kernels_share_of_measured_hbm"] = (patch_bytes + dct_bytes) / (patch_ms[0] + dct_ms[0]) / 1e6 / HBM_MEASURED_GBS
    # (d) the photometric stage
    staged_chain = ssd_augment.SSDDataAugmentation(OUT, OUT, photometric_distortions=ssd_augment.SSDPhotometricDistortions())

    def plan_all_photometric():
        np.random.seed(1)
        out = [staged_chain.plan(im.shape[0], im.shape[1], y, return_photometric=True) for im, y in zip(images, labels)]
        return [o[0] for o in out], [o[-1] for o in out]
    geometries_p, records = plan_all_photometric()
    res["photometric_ops_per_image"] = float(np.mean([sum(v is not None for v in r[1:5]) for r in records]))
    res["photometric_host_ms"] = median_ms(
        lambda: list(pool.map(lambda a: ssd_augment.ssd_photometric_host(*a), zip(images, records))), max(5, args.reps // 2))

    def device_photometric():
        g, r = plan_all_photometric()
        prep(images, g, photometric=r).emit_into(bufs)
    res["device_photometric_ms"] = median_ms(device_photometric, args.reps)
    pending_p = prep(images, geometries_p, photometric=records)
    res["device_photometric_emit_only_ms"] = median_ms(lambda: pending_p.emit_into(bufs), args.reps)
    res["device_photometric_equals_host"] = all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(bufs, pending_p.numpy()))
    plan_p = pending_p.plan
    staging_p = torch.empty(plan_p.nbytes, dtype=torch.uint8).pin_memory()
    plan_p.fill(staging_p.numpy(), images)
    host_p = staging_p.numpy()
    blob_p = staging_p.to(dev)
    src_d, desc_d, _ = plan_p.views(blob_p)
    _, desc_h, _ = plan_p.views(host_p)
    # in place, over and over on the same bytes: the work per pixel does not depend on their values
    photo_ms = event_ms(lambda: kernels.ssd_photometric(src_d, desc_d, desc_h, plan_p.photo_view(blob_p), plan_p.photo_view(host_p)),
                        reps)
    dp = plan_p.desc
    photo_bytes = int(2 * (dp["src_h"].astype(np.int64) * dp["src_w"] * 3).sum())
    res["ssd_photometric_ms"], res["ssd_photometric_bytes"] = photo_ms, photo_bytes
    res["ssd_photometric_GBs"] = photo_bytes / photo_ms[0] / 1e6
    scratch_p = torch.empty(plan_p.scratch_bytes, dtype=torch.uint8, device=dev)
    res["photometric_plus_patch_resize_ms"] = event_ms(lambda: plan_p.launch(host_p, blob_p, pixels, scratch_p), reps)
    res["mean_taps"] = [float(np.mean([plan.pool[int(x["h_bounds"]) + 1:int(x["h_bounds"]) + 2 * OUT:2].mean() for x in d])),
                        float(np.mean([plan.pool[int(x["v_bounds"]) + 1:int(x["v_bounds"]) + 2 * OUT:2].mean() for x in d]))]
    res["h_grid_fill"] = float(rows.mean() / rows.max())      # share of the horizontal pass's blocks that have work
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
