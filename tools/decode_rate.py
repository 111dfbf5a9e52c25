"""Cost of getting one batch of JPEG FILES (32 PIL-written files of mixed sizes around 375x500, quality 90, 4:2:0) into the
staged pixel rectangles that dj_patch_resize reads, decoding on the host against decoding the pixel half on the GPU, with
the geometries drawn by `SSDDataAugmentation.plan` under a fixed seed (the batch and seed of tools/ssd_input_rate.py):

  (i)   the parent's path: Pillow's full decode of every file, one after the other in the calling thread (what
        `DataGeneratorDCT.generate` does per batch), then `PatchPlan.fill` of the decoded arrays into pinned memory
        (`pillow_decode_ms`, `fill_arrays_ms`, and their sum in one window `host_decode_path_ms`)
  (ii)  the new path: the files' headers read for planning (`CoefficientImage` per file, `headers_ms`), then
        `PatchPlan.fill`, whose batch reader entropy-decodes the raw coefficient planes on 16 threads, each into planes
        of its own that it copies to their place in the pinned blob (`fill_coefficients_ms`; `--threads` for another
        count; `fill_coefficients_1_thread_ms` beside it), and their sum in one window (`coefficient_path_ms`)
  (iii) the kernels, by device events, two ways: ONE call between two events (`*_call_ms`: the ctypes call, the host-side
        validation of 32 descriptors and launch latency are inside, so for launches this small it is a latency, not a
        kernel time), and 50 calls back to back between two events, per call (`*_ms`: host issue and GPU execution overlap,
        so it is the larger of the two per call -- an upper bound of the kernels' time, and the rate a training loop
        sees).  dj_jpeg_pixels on the staged batch, with the bytes it reads and writes once each, beside dj_patch_resize
        on the same batch, both in one `launch`, and the pinned upload of either blob

    python tools/decode_rate.py [--reps 20] [--threads 16]

Medians over `reps` after warm-up, with min and max; every timed window that launches ends in a device synchronise.
`pixels_equal` confirms that both paths leave the same uint8 batch.  Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd.data import patch_resize, ssd_augment
from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage

OUT = 300


def host_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, reps, inner=1):
    """Device time between two events around `inner` calls of `fn`, per call."""
    for _ in range(5):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return statistics.median(times), min(times), max(times)


def make_files(rng, n):
    """The batch of tools/ssd_input_rate.py (smooth content plus noise, sides within +-15 % of 375 x 500, two to four
    boxes each), written as JPEG files by PIL."""
    from PIL import Image
    files, labels = [], []
    for i in range(n):
        h, w = int(375 * rng.uniform(0.85, 1.15)), int(500 * rng.uniform(0.85, 1.15))
        if i % 3 == 2:
            h, w = w, h
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / (11.0 + c + i % 7) + c) * np.cos(yy / (8.0 + 2 * c)) for c in range(3)], axis=-1)
        buf = io.BytesIO()
        Image.fromarray(np.clip(img + rng.normal(0, 15, img.shape), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90)
        files.append(buf.getvalue())
        rows = []
        for _ in range(int(rng.integers(2, 5))):
            bw, bh = int(rng.integers(40, w // 2)), int(rng.integers(40, h // 2))
            x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            rows.append([int(rng.integers(1, 21)), x0, y0, x0 + bw, y0 + bh])
        labels.append(np.array(rows))
    return files, labels


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as image:
        return np.array(image.convert("RGB"), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    B = 32
    files, labels = make_files(np.random.default_rng(0), B)
    coefficient = [CoefficientImage(f) for f in files]
    arrays = [pillow_decode(f) for f in files]
    chain = ssd_augment.SSDDataAugmentation(OUT, OUT)
    np.random.seed(1)
    geometries = [chain.plan(im.shape[0], im.shape[1], y)[0] for im, y in zip(arrays, labels)]
    import PIL
    res = {"batch": B, "reps": args.reps, "threads": args.threads, "pil": PIL.__version__,
           "file_MB": sum(len(f) for f in files) / 1e6, "pixel_MB": sum(a.nbytes for a in arrays) / 1e6}
    prep = patch_resize.DevicePatchResize(OUT, OUT, deconv=True)
    plan_a = prep(arrays, geometries).plan
    plan_c = prep(coefficient, geometries).plan
    staging_a = torch.empty(plan_a.nbytes, dtype=torch.uint8).pin_memory()
    staging_c = torch.empty(plan_c.nbytes, dtype=torch.uint8).pin_memory()
    host_a, host_c = staging_a.numpy(), staging_c.numpy()
    res["blob_arrays_MB"], res["blob_coefficients_MB"] = plan_a.nbytes / 1e6, plan_c.nbytes / 1e6
    res["coefficient_MB"] = plan_c.coef_bytes / 1e6

    # (i) the parent's path
    res["pillow_decode_ms"] = host_ms(lambda: [pillow_decode(f) for f in files], args.reps)
    res["fill_arrays_ms"] = host_ms(lambda: plan_a.fill(host_a, arrays), args.reps)
    res["host_decode_path_ms"] = host_ms(lambda: plan_a.fill(host_a, [pillow_decode(f) for f in files]), args.reps)
    # (ii) the new path
    res["headers_ms"] = host_ms(lambda: [CoefficientImage(f) for f in files], args.reps)
    res["fill_coefficients_ms"] = host_ms(lambda: plan_c.fill(host_c, coefficient, n_threads=args.threads), args.reps)
    res["fill_coefficients_1_thread_ms"] = host_ms(lambda: plan_c.fill(host_c, coefficient, n_threads=1), max(5, args.reps // 2))
    res["coefficient_path_ms"] = host_ms(
        lambda: plan_c.fill(host_c, [CoefficientImage(f) for f in files], n_threads=args.threads), args.reps)
    res["parent_over_new"] = res["host_decode_path_ms"][0] / res["coefficient_path_ms"][0]

    # (iii) the kernels alone, and the uploads
    def upload(staging):
        staging.to(dev, non_blocking=True)
        torch.cuda.synchronize()
    res["upload_arrays_ms"] = host_ms(lambda: upload(staging_a), args.reps)
    res["upload_coefficients_ms"] = host_ms(lambda: upload(staging_c), args.reps)
    blob_a, blob_c = staging_a.to(dev), staging_c.to(dev)
    scratch = torch.empty(plan_c.scratch_bytes, dtype=torch.uint8, device=dev)
    pixels_a = torch.empty(plan_a.out_shape, dtype=torch.uint8, device=dev)
    pixels_c = torch.empty(plan_c.out_shape, dtype=torch.uint8, device=dev)
    reps = max(50, args.reps)
    for name, fn in (("jpeg_pixels", lambda: plan_c.launch_decode(host_c, blob_c, scratch)),
                     ("patch_resize", lambda: plan_a.launch(host_a, blob_a, pixels_a, scratch)),
                     ("jpeg_pixels_plus_patch_resize", lambda: plan_c.launch(host_c, blob_c, pixels_c, scratch))):
        res[name + "_call_ms"] = event_ms(fn, reps)
        res[name + "_ms"] = event_ms(fn, args.reps, inner=50)
        t0 = time.perf_counter()
        for _ in range(200):
            fn()
        res[name + "_host_issue_ms"] = (time.perf_counter() - t0) * 1e3 / 200      # host time per call while the queue takes them
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    res["pixels_equal"] = bool(torch.equal(pixels_a, pixels_c))
    d = plan_c.decode
    blocks = ((d["by1"] - d["by0"]).astype(np.int64) * (d["bx1"] - d["bx0"])).sum()
    rect = ((d["yb"] - d["ya"]).astype(np.int64) * (d["xb"] - d["xa"])).sum()
    # coefficients read, sample planes written and read, pixels written
    jpx_bytes = int(blocks * 128 + 2 * blocks * 64 + 3 * rect)
    # at least this rate: `jpeg_pixels_ms` is an upper bound of the kernels' time
    res["jpeg_pixels_bytes"], res["jpeg_pixels_GBs_at_least"] = jpx_bytes, jpx_bytes / res["jpeg_pixels_ms"][0] / 1e6
    res["blocks_share_of_planes"] = float(blocks * 128 / sum(int(c) for c in plan_c.plane_capacity.reshape(-1) * 2))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
