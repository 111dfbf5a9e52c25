"""keras.metrics.top_k_categorical_accuracy as the reference's configs use it
(classification_part/config/resnet/config_file.py:19-22): evaluated with torch on the device-resident batch."""
import torch


def top_k_categorical_accuracy(y_true, y_pred, k=5):
    y_true = torch.as_tensor(y_true)
    y_pred = torch.as_tensor(y_pred).to(y_true.device)
    target = y_true.argmax(dim=-1)
    topk = y_pred.topk(k, dim=-1).indices
    return float((topk == target.unsqueeze(-1)).any(dim=-1).float().mean())


def categorical_accuracy(y_true, y_pred):
    return top_k_categorical_accuracy(y_true, y_pred, 1)


# ---- validation sweeps: what the device accumulator (dj_eval_accumulate) counts, and which metrics it can take -----------------
def classification_counts_host(y_true, probs, ks):
    """-> int64 array [1 + len(ks)]: the number of rows, then the hits of every entry of `ks` over the [rows][C] batch.
    The target is t = np.argmax(y_true[row]) (first maximum, a NaN counts as the maximum) and p_t = probs[row][t].  An
    entry k >= 1 is tf.nn.in_top_k, which Keras 2.2.4's top_k_categorical_accuracy calls: a hit iff p_t is finite and
    fewer than k classes lie strictly above it (classes tied with the target all count as in the top k; a NaN compares
    false).  An entry 0 is categorical_accuracy: a hit iff np.argmax(probs[row]) == t.  This is the statement the kernel's
    counts equal exactly."""
    import numpy as np
    y_true, probs = np.asarray(y_true, dtype=np.float32), np.asarray(probs, dtype=np.float32)
    out = np.zeros(1 + len(ks), dtype=np.int64)
    out[0] = probs.shape[0]
    if probs.shape[0] == 0:
        return out
    t = np.argmax(y_true, axis=-1)
    p_t = probs[np.arange(probs.shape[0]), t]
    with np.errstate(invalid="ignore"):
        above = (probs > p_t[:, None]).sum(-1)
    for q, k in enumerate(ks):
        if k == 0:
            out[1 + q] = int((np.argmax(probs, axis=-1) == t).sum())
        else:
            out[1 + q] = int((np.isfinite(p_t) & (above < k)).sum())
    return out


def device_metric_k(metric):
    """-> the `ks` entry under which the sweep's kernel counts `metric` (k >= 1: top-k accuracy, 0: categorical accuracy), or
    None when it has to be evaluated per batch as metric(y_true, y_pred).  Taken are 'accuracy' / 'acc', the two functions
    of this module themselves, and a callable that carries `_dj_metric = ("top_k", k)`."""
    if isinstance(metric, str):
        return 0 if metric in ("accuracy", "acc") else None
    if metric is top_k_categorical_accuracy:
        return 5
    if metric is categorical_accuracy:
        return 0
    tag = getattr(metric, "_dj_metric", None)
    if isinstance(tag, tuple) and len(tag) == 2 and tag[0] == "top_k" and isinstance(tag[1], int) and tag[1] >= 1:
        return int(tag[1])
    return None


def metric_entries(metrics):
    """-> [(log name, metric callable)] for a compile-time `metrics` list: the names Model._metric_values gives its values
    (Keras names anonymous metric functions `_func`, `_func_1`, ...; 'accuracy' is 'acc'; unknown strings are dropped)."""
    out, seen = [], {}
    for m in metrics:
        name = getattr(m, "__name__", str(m)) if callable(m) else str(m)
        if not callable(m):
            if name not in ("accuracy", "acc"):
                continue
            name = "acc"
        n = seen.get(name, 0)
        seen[name] = n + 1
        out.append((name if n == 0 else "%s_%d" % (name, n), m))
    return out
