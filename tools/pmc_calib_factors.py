"""(fetch.csv, write.csv of a tools/pmc_calibrate.py run) -> 'F32_FETCH F32_WRITE F16_FETCH F16_WRITE' scale factors.
dj_copy2d and dj_copy2d_t launch two instances of one template, dj_copy2d_kernel<VEC, TYPED>: the trace tells them apart
by the second template argument (`false`: the fp32 code of dj_copy2d, `true`: the type-carrying code of dj_copy2d_t)."""
import csv, re, sys
def per_launch(path, counter, typed):
    inst = re.compile(r"dj_copy2d_kernel<\d+, %s>" % ("true" if typed else "false"))
    v = [float(r["Counter_Value"]) * 1024.0 for r in csv.DictReader(open(path)) if r["Counter_Name"] == counter and inst.search(r["Kernel_Name"])]
    assert v, "no dj_copy2d_kernel<.., %s> launch with %s in %s" % (str(typed).lower(), counter, path)
    return sum(v) / len(v)
f, w = sys.argv[1], sys.argv[2]
n32, n16 = (1 << 28) * 4.0, (1 << 28) * 2.0
print("%.4f %.4f %.4f %.4f" % (n32 / per_launch(f, "FETCH_SIZE", False), n32 / per_launch(w, "WRITE_SIZE", False),
                               n16 / per_launch(f, "FETCH_SIZE", True), n16 / per_launch(w, "WRITE_SIZE", True)))
