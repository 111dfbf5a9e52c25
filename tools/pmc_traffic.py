"""HBM traffic per implicit-GEMM launch from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; KB units).
gfx950 correction (MI355X_MICROARCH.md, HBM section): FETCH_SIZE counts 128-B requests of 16-B-per-lane loads at
64 B -> doubled; WRITE_SIZE taken as is.  Only the launches of the LAST training step are used (autotune and warm-up
launches come first in the trace)."""
import csv, sys, json, collections

def last_step(path, counter):
    rows = [r for r in csv.DictReader(open(path)) if r["Counter_Name"] == counter]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    marks = [i for i, r in enumerate(rows) if "dj_ssd_loss_bwd" in r["Kernel_Name"]]
    fwd0 = [i for i, r in enumerate(rows) if "dj_softmax_fwd" in r["Kernel_Name"]]
    # one step = from the sgd of the previous step to the sgd of this one
    sgd = [i for i, r in enumerate(rows) if "dj_optim_kernel" in r["Kernel_Name"] or "dj_sgd" in r["Kernel_Name"]]
    hi = sgd[-1]
    lo = max(i for i in sgd if i < marks[-1] and i < fwd0[-1]) + 1 if any(i < fwd0[-1] for i in sgd) else 0
    return rows[lo:hi + 1]

fetch = last_step(sys.argv[1], "FETCH_SIZE")
write = last_step(sys.argv[2], "WRITE_SIZE")
# optional: counter scale factors measured by tools/pmc_calibrate.py on this box (known bytes / reported bytes), e.g. for
# the float16 mode's 8-byte-per-lane accesses:  pmc_traffic.py fetch.csv write.csv out.json FETCH_SCALE WRITE_SCALE
FETCH_SCALE = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
WRITE_SCALE = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
def agg(rows, scale):
    d = collections.defaultdict(lambda: [0, 0.0])
    for r in rows:
        fam = "igemm" if "dj_igemm" in r["Kernel_Name"] else r["Kernel_Name"].split("(")[0].replace("void ", "")[:60]
        d[fam][0] += 1; d[fam][1] += float(r["Counter_Value"]) * 1024.0 * scale
    return d
f, w = agg(fetch, FETCH_SCALE), agg(write, WRITE_SCALE)
out = {}
print("%-62s %6s %12s %12s" % ("kernel family (last step)", "calls", "fetch MB", "write MB"))
for k in sorted(set(f) | set(w), key=lambda k: -(f.get(k, [0, 0])[1] + w.get(k, [0, 0])[1])):
    print("%-62s %6d %12.1f %12.1f" % (k, f.get(k, [0, 0])[0], f.get(k, [0, 0])[1] / 1e6, w.get(k, [0, 0])[1] / 1e6))
ig_calls = f["igemm"][0]
out = dict(kernel="dj_igemm*", launches_per_step=ig_calls, fetch_bytes_per_step=f["igemm"][1], write_bytes_per_step=w["igemm"][1],
           bytes_per_launch=(f["igemm"][1] + w["igemm"][1]) / ig_calls,
           step_total_bytes=sum(v[1] for v in f.values()) + sum(v[1] for v in w.values()),
           note="FETCH_SIZE x%.3f, WRITE_SIZE x%.3f (x2 / x1: the guide's gfx950 correction for 16-B-per-lane accesses; other values: "
                "calibrated on this box with tools/pmc_calibrate.py for the access width of the mode), KB units x1024" % (FETCH_SCALE, WRITE_SCALE))
print(json.dumps(out))
if len(sys.argv) > 3:
    json.dump(out, open(sys.argv[3], "w"), indent=1)
