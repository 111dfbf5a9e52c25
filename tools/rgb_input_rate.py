"""Cost of one batch of the RGB ResNet50's input pipeline -- 64 image files around 375x500, loaded at 224x224 and put
through the reference's training arguments (ImageDataGenerator(featurewise_center=True, rotation_range=0.2,
shear_range=0.2, zoom_range=0.2, vertical_flip=True, preprocessing_function=preprocess_input)) -- host path vs device path:

  (i)  host:   flow_from_directory(...)[k]: PIL decode + nearest resize, the in-tree numpy warp (data/rgb_warp.py), flips,
               preprocess_input; its warp part alone; and, where scipy imports, the same warp done as Keras does it
               (scipy.ndimage.affine_transform once per channel), per batch and per image, one thread
  (ii) device: flow_from_directory(..., device_prep=True)[k] (decode + resize + draws on the host), the upload of pixels
               and records from pinned memory, and dj_rgb_warp by device events around 50 back-to-back launches, with the
               bytes it moves over that time
  (iii) device decode: flow_from_directory(..., device_prep=True, device_decode=True)[k] (files read, headers, draws and
               the plan; nothing decoded or resized on the host), `fill` of the blob with the coefficient read on 16
               threads and on 1, the upload of that blob, the kernels by device events (dj_jpeg_pixels + dj_patch_resize,
               then dj_rgb_warp) and the whole `emit_into`; the output asserted equal to (ii)'s

    python tools/rgb_input_rate.py [--reps 5] [--dir DIRECTORY]

Medians over `reps` after a warm-up; every timed window ends in a device synchronise where the device takes part.  There is
no target: the device path is compared with the host path of the same run on the same machine, and device decode with the
device path of the same run.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import kernels
from jpeg_detection_resnet_ssd_amd.data import rgb_warp
from jpeg_detection_resnet_ssd_amd.keras.applications.vgg16 import preprocess_input
from jpeg_detection_resnet_ssd_amd.keras.preprocessing.image import ImageDataGenerator

HBM_MEASURED_GBS = 6290.0     # float4 copy on MI355X (tools/input_rate.py)
T, B = 224, 64
TRAIN_ARGS = dict(featurewise_center=True, rotation_range=0.2, shear_range=0.2, zoom_range=0.2, vertical_flip=True,
                  validation_split=0, preprocessing_function=preprocess_input)


def write_files(root, n, rng):
    """Smooth content plus noise, landscape and portrait, sides within +-15 % of 375 x 500, as JPEG in 4 class directories."""
    from PIL import Image
    for i in range(n):
        h, w = int(375 * rng.uniform(0.85, 1.15)), int(500 * rng.uniform(0.85, 1.15))
        if i % 3 == 2:
            h, w = w, h
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / (11.0 + c + i % 7) + c) * np.cos(yy / (8.0 + 2 * c)) for c in range(3)], axis=-1)
        img = np.clip(img + rng.normal(0, 15, img.shape), 0, 255).astype(np.uint8)
        directory = os.path.join(root, "class%d" % (i % 4))
        os.makedirs(directory, exist_ok=True)
        Image.fromarray(img).save(os.path.join(directory, "img%03d.jpg" % i), quality=90)


def median_ms(fn, reps, warmup=1, sync=False):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, reps, inner=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / inner)
    return statistics.median(windows), min(windows), max(windows)


def decode_rows(res, iterator, want, dev, reps):
    """Row (iii).  `want`: the tensor (ii) wrote for the same seed."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    its = {n: iterator(True, device_decode=True, decode_threads=n) for n in (16, 1)}
    res["decode_host_part_ms"] = median_ms(lambda: its[16][0], reps)          # read, headers, draws, records, plan
    out = torch.empty((B, T, T, 3), dtype=torch.float32, device=dev)
    pending = iterator(True, device_decode=True, decode_threads=16)[0][0]     # a fresh iterator: the same seed, the same draws
    assert all(isinstance(im, CoefficientImage) for im in pending.images), "every file must travel as coefficients"
    plan = pending.plan
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    for n in (16, 1):
        res["decode_fill_%d_threads_ms" % n] = median_ms(lambda: plan.fill(host, pending.images, n), max(10, reps), warmup=2)
        res["decode_batch_%d_threads_ms" % n] = median_ms(lambda: its[n][0][0].emit_into([out]), reps, sync=True)
    res["decode_emit_ms"] = median_ms(lambda: pending.emit_into([out]), max(20, reps), warmup=3, sync=True)
    res["device_decode_equals_device_prep"] = bool(torch.equal(out, want))
    assert res["device_decode_equals_device_prep"], "device decode and device prep disagree"
    res["decode_upload_MB"] = plan.nbytes / 1e6
    res["decode_upload_ms"] = median_ms(lambda: staging.to(dev, non_blocking=True), max(20, reps), warmup=3, sync=True)
    blob = staging.to(dev)
    pixels = torch.empty(plan.out_shape, dtype=torch.uint8, device=dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    rec_dev = plan.part(blob, plan.records_offset, pending.records)
    res["decode_jpeg_pixels_ms"] = event_ms(lambda: plan.launch_decode(host, blob, scratch), max(5, reps))
    res["decode_pixels_resize_ms"] = event_ms(lambda: plan.launch(host, blob, pixels, scratch), max(5, reps))
    res["decode_kernels_ms"] = event_ms(lambda: (plan.launch(host, blob, pixels, scratch),
                                                 kernels.rgb_warp(pixels, rec_dev, pending.records, out, pending.preprocess, None)),
                                        max(5, reps))
    res["device_batch_over_decode_batch"] = res["device_batch_ms"][0] / res["decode_batch_16_threads_ms"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="write the files here (default: a temporary directory)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rgb_input_rate.py measures on the GPU"
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")          # the unfit featurewise_center warning of the reference's call
    tmp = None
    if args.dir is None:
        tmp = tempfile.TemporaryDirectory()
    root = args.dir or tmp.name
    write_files(root, B, np.random.default_rng(0))
    res = {"batch": B, "target": T, "reps": args.reps}

    def iterator(device_prep, **kw):
        return ImageDataGenerator(**TRAIN_ARGS).flow_from_directory(root, target_size=(T, T), batch_size=B, seed=1,
                                                                    device_prep=device_prep, **kw)
    host_it, dev_it = iterator(False), iterator(True)
    # (i) the host path
    res["host_batch_ms"] = median_ms(lambda: host_it[0], args.reps)
    pending, want = iterator(True)[0][0], iterator(False)[0][0]      # fresh iterators: the same seed, the same draws
    records = [rec["m"].reshape(2, 3) for rec in pending.records]
    res["host_warp_numpy_ms"] = median_ms(lambda: [rgb_warp.affine_warp_host(p, m) for p, m in zip(pending.pixels, records)],
                                          args.reps)
    try:
        from scipy import ndimage
        import scipy

        def keras_warp():
            for p, m in zip(pending.pixels, records):
                x = np.rollaxis(p.astype(np.float32), 2, 0)
                np.rollaxis(np.stack([ndimage.affine_transform(ch, m[:, :2], m[:, 2], order=1, mode="nearest", cval=0.)
                                      for ch in x], axis=0), 0, 3)
        res["scipy"] = scipy.__version__
        res["host_warp_scipy_ms"] = median_ms(keras_warp, args.reps)
        res["host_warp_scipy_ms_per_image"] = res["host_warp_scipy_ms"][0] / B
    except ImportError:
        res["scipy"] = False
        res["host_warp_scipy_ms"] = "not measured (no scipy)"
    # (ii) the device path
    res["device_host_part_ms"] = median_ms(lambda: dev_it[0], args.reps)          # decode, resize, draws, records
    out = torch.empty((B, T, T, 3), dtype=torch.float32, device=dev)
    res["device_emit_ms"] = median_ms(lambda: pending.emit_into([out]), max(20, args.reps), warmup=3, sync=True)
    res["device_equals_host"] = bool(np.array_equal(out.cpu().numpy(), want))
    res["device_batch_ms"] = median_ms(lambda: dev_it[0][0].emit_into([out]), args.reps, sync=True)
    pending.emit_into([out])
    torch.cuda.synchronize()
    decode_rows(res, iterator, out.clone(), dev, args.reps)
    stager = rgb_warp.RGBWarpStager()
    res["upload_ms"] = median_ms(lambda: stager.upload(pending.pixels, pending.records, dev), max(20, args.reps), warmup=3,
                                 sync=True)
    res["upload_MB"] = (pending.pixels.nbytes + pending.records.nbytes) / 1e6
    pix_dev, rec_dev = stager.upload(pending.pixels, pending.records, dev)

    def launch():
        kernels.rgb_warp(pix_dev, rec_dev, pending.records, out, pending.preprocess, None)
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    windows = []
    for _ in range(max(5, args.reps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / 50)
    res["kernel_ms"] = (statistics.median(windows), min(windows), max(windows))
    moved = pix_dev.numel() + out.numel() * 4 + pending.records.nbytes      # the source is read once from HBM, gathers hit cache
    res["kernel_bytes"], res["kernel_GBs"] = moved, moved / res["kernel_ms"][0] / 1e6
    res["kernel_share_of_measured_hbm"] = res["kernel_GBs"] / HBM_MEASURED_GBS
    res["host_over_device_batch"] = res["host_batch_ms"][0] / res["device_batch_ms"][0]
    res["host_warp_numpy_over_device_emit"] = res["host_warp_numpy_ms"][0] / res["device_emit_ms"][0]
    print(json.dumps(res), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
