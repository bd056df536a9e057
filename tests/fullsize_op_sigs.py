"""Signatures of the public ops a full-size training step calls (test infrastructure; imports without a GPU).

`Recorder` wraps `ops.<name>` for every op in RECORDED while a step runs (the modeling code reaches them only through
`ops.<name>`, and calls inside ops.py resolve the module attribute too) and records, per call, a signature: the op, the
tensor shapes, the actual sequence lengths / row masks and the flags that select a kernel path.  A signature is a tuple
(op, ((field, value), ...)) of plain Python values, so the table of tests/test_fullsize_ops_gpu.py can hold them literally."""
import math

RECORDED = ("linear", "linear_group", "linear_kn", "conv3", "layernorm", "dwconv3", "maxpool3s2", "scale_add", "axpby",
            "add_pe", "attention", "rel_attention", "channel_attention", "qkv_pre", "bias_add", "colsum", "transpose",
            "permute3", "dropout")

# what the step also runs, and where it is held to a float64 (or bit-exact) reference instead
EXEMPT = {
    "mq_loss": "tests/test_loss_gpu.py and the loss goldens",
    "optimizer": "tests/test_train_utils.py",
    "pack / pack_many / pack_tap / weight_planes": "the operand planes: tests/test_step_gemm_census_gpu.py decodes every one a GEMM reads",
    "decode / NMS": "not part of the training step (tests/test_nms_gpu.py; the decode at its edges and at the recipe's shape: "
                    "tests/test_decode_edges_gpu.py against tests/decode_restatement.py)",
}


def _shape(t):
    return None if t is None else tuple(int(s) for s in t.shape)


def _vals(t):
    """actual lengths (a device int tensor or a list) as a tuple"""
    if t is None:
        return None
    if hasattr(t, "tolist"):
        return tuple(int(v) for v in t.reshape(-1).tolist())
    return tuple(int(v) for v in t)


def _rle(m):
    """a 0 / 1 row mask as run lengths ((value, count), ...)"""
    if m is None:
        return None
    out = []
    for v in m.reshape(-1).tolist():
        v = int(v != 0)
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return tuple(tuple(r) for r in out)


def _f(x):
    return None if x is None else float(x)


def _rg(*ts):
    return tuple(bool(t is not None and getattr(t, "requires_grad", False)) for t in ts)


def _sig_linear(x, w, b=None, act=0, lens=None, T=None, drop_p=0.0, drop_site="dropout", bwd_precision=None):
    return dict(x=_shape(x), w=_shape(w), bias=b is not None, act=int(act), lens=_vals(lens), T=None if T is None else int(T),
                drop_p=float(drop_p), bwd_precision=bwd_precision, rg=_rg(x, w, b))


def _sig_linear_group(xs, ws, bs):
    return dict(n=len(xs), x=_shape(xs[0]), w=_shape(ws[0]), bias=all(b is not None for b in bs), rg=_rg(xs[0], ws[0]))


def _sig_linear_kn(x, w, b=None):
    return dict(x=_shape(x), w=_shape(w), bias=b is not None, rg=_rg(x, w, b))


def _sig_conv3(x, w, b=None, lens=None, row_mask=None):
    return dict(x=_shape(x), w=_shape(w), bias=b is not None, lens=_vals(lens), row_mask=_rle(row_mask), rg=_rg(x, w, b))


def _sig_layernorm(x, gamma, beta, eps=1e-5, relu=False, planes=None, row_mask=None, skip=False, site=None):
    return dict(x=_shape(x), eps=float(eps), relu=bool(relu), planes=planes, row_mask=_rle(row_mask), skip=bool(skip),
                rg=_rg(x, gamma, beta))


def _sig_dwconv3(x, w, lens, stride):
    return dict(x=_shape(x), lens=_vals(lens), stride=int(stride), rg=_rg(x, w))


def _sig_maxpool3s2(x, lens):
    return dict(x=_shape(x), lens=_vals(lens), rg=_rg(x))


def _sig_scale_add(a, b, colscale=None, rowscale=None, lens=None, mask_a=False):
    return dict(a=_shape(a), b=_shape(b), colscale=_shape(colscale), rowscale=_shape(rowscale), lens=_vals(lens),
                mask_a=bool(mask_a), rg=_rg(a, b, colscale, rowscale))


def _sig_axpby(a, b, alpha, beta):
    return dict(a=_shape(a), b=_shape(b), alpha=float(alpha), beta=float(beta), rg=_rg(a, b))


def _sig_add_pe(x, pe_tm, lens):
    return dict(x=_shape(x), pe=_shape(pe_tm), lens=_vals(lens), rg=_rg(x, pe_tm))


def _sig_attention(q, k, v, kv_len, n_head, scale=None, mode=0, drop_p=0.0, window=0):
    from vilco_amd import ops
    hd = q.shape[-1] // n_head
    return dict(q=_shape(q), k=_shape(k), kv_len=_vals(kv_len), H=int(n_head),
                scale=float(1.0 / math.sqrt(hd) if scale is None else scale), mode=int(mode), drop_p=float(drop_p),
                window=int(window), flash=bool(ops.use_flash and ops.flash_supported(hd)), rg=_rg(q, k, v))


def _sig_rel_attention(qw, qr, k, v, kr, kv_len, n_head, scale, drop_p=0.0):
    from vilco_amd import ops
    return dict(q=_shape(qw), kr=_shape(kr), kv_len=_vals(kv_len), H=int(n_head), scale=float(scale), drop_p=float(drop_p),
                flash=bool(ops.use_flash and ops.flash_supported(qw.shape[-1] // n_head)), rg=_rg(qw, qr, k, v, kr))


def _sig_channel_attention(qkv, n_head, scale, bwd_precision=None):
    return dict(qkv=_shape(qkv), H=int(n_head), scale=float(scale), bwd_precision=bwd_precision, rg=_rg(qkv))


def _sig_qkv_pre(x, ln1, convs, norms, lens, stride, want_h, skip=False):
    return dict(x=_shape(x), lens=_vals(lens), stride=int(stride), want_h=bool(want_h), skip=bool(skip),
                eps=(float(ln1[2]), float(norms[3])), rg=_rg(x))


def _sig_bias_add(x, b):
    return dict(x=_shape(x), b=_shape(b), rg=_rg(x, b))


def _sig_colsum(x2d, param=None):
    return dict(x=_shape(x2d))


def _sig_transpose(x):
    return dict(x=_shape(x), rg=_rg(x))


def _sig_permute3(src, dims, off, strides, out=None):
    return dict(src=_shape(src), dims=tuple(int(d) for d in dims), off=int(off), strides=tuple(int(s) for s in strides))


def _sig_dropout(x, p, training, site="dropout"):
    return dict(x=_shape(x), p=float(p), training=bool(training), site=site, rg=_rg(x))


SIG = {name: globals()["_sig_" + name] for name in RECORDED}


def freeze(op, d):
    return (op, tuple(sorted(d.items())))


class Recorder:
    """with Recorder(monkeypatch) as rec: ... -> rec.seen: {signature: calls}"""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch
        self.seen = {}

    def __enter__(self):
        from vilco_amd import ops
        for name in RECORDED:
            real, sig = getattr(ops, name), SIG[name]

            def wrapped(*a, _real=real, _sig=sig, _name=name, **k):
                key = freeze(_name, _sig(*a, **k))
                self.seen[key] = self.seen.get(key, 0) + 1
                return _real(*a, **k)
            self.mp.setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False
