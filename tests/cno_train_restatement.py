"""Plain-torch fp64 restatement of the CNO3d training step (a plain module, not a test file): forward with batch-statistics BatchNorm and
the running-statistics update, and the backward pass as the kernels compute it -- no autograd.

Per layer on rows [M][C] (M = B * T * H * W):
    forward    y = conv(x) + bias;  mean, var (biased) over M;  a = gamma / sqrt(var + eps), b = beta - mean a;  z = y a + b;
               v = act ? lrelu(z) : z;  v += res
               running_mean = 0.9 rm + 0.1 mean;  running_var = 0.9 rv + 0.1 var M / (M - 1);  num_batches_tracked += 1
    backward   dz = gv (z > 0 ? 1 : 0.2);  dbeta = sum dz;  dgamma = sum dz xhat, xhat = (y - mean) rstd;
               dy = a (dz - dbeta / M - xhat dgamma / M);  without BatchNorm dy = dz
               dW[co][ci][tap] = sum_m dy[m][co] x[m + tap - 1][ci];  db = sum_m dy (the bias in front of a BatchNorm included: ~0)
               dx = the same convolution of dy with the flipped, transposed taps Wd[ci][co][tap] = W[co][ci][2 - tap]
The data flow is that of tests/cno_restatement.py: a concat is two producers writing column ranges of one buffer (its gradient: two
layers reading column ranges of one gradient buffer), a residual hands its gradient to the block input unchanged, the first consumer of
a buffer writes its gradient and later ones add to it, the neck runs in reverse index order."""
import torch
import torch.nn.functional as F

from cno_restatement import WIDTHS

EPS, MOMENTUM = 1e-5, 0.1


def conv_rows(rows, w, B, mesh):
    """rows [M][Ci], w [Co][Ci][3][3][3] -> [M][Co] (padding 1)"""
    T, H, W = mesh
    return F.conv3d(rows.view(B, T, H, W, -1).permute(0, 4, 1, 2, 3), w, padding=1).permute(0, 2, 3, 4, 1).reshape(rows.shape[0], -1)


def flipped(w):
    """[Co][Ci][3][3][3] -> the data-gradient weights [Ci][Co][3][3][3]"""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def weight_grad(dy, rows, B, mesh):
    """dW [Co][Ci][3][3][3] from dy [M][Co] and the layer's input rows [M][Ci]"""
    T, H, W = mesh
    Co, Ci = dy.shape[1], rows.shape[1]
    xp = F.pad(rows.view(B, T, H, W, Ci), (0, 0, 1, 1, 1, 1, 1, 1))
    dW = torch.zeros(Co, Ci, 3, 3, 3, dtype=dy.dtype)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                dW[:, :, kt, kh, kw] = dy.t() @ xp[:, kt:kt + T, kh:kh + H, kw:kw + W, :].reshape(-1, Ci)
    return dW


class _Buf:
    def __init__(self, M, width):
        self.v = torch.zeros(M, width, dtype=torch.float64)


def train_step(sd, x, target, tape_out=None):
    """(out, loss, stats, grads): ``out`` [B, *shape_out], ``loss`` the mean squared error, ``stats`` {name: updated running statistic or
    counter}, ``grads`` {parameter name: gradient} of ``loss`` -- all fp64; ``sd``: a reference ``state_dict``, x [B][T][H][W][C] (C < T).
    ``tape_out`` (a list) receives the per-layer records (``conv``, ``act``, ``z``, ``y`` ...) in forward order."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x, target = x.double(), target.double()
    B, T, H, W, C = x.shape
    assert C < T
    mesh, M = (T, H, W), B * T * H * W
    tape, stats, grads = ([] if tape_out is None else tape_out), {}, {}

    def layer(conv, bn, src, dst=None, col=0, act=True, res=None):
        w, bias = sd[conv + ".weight"], sd[conv + ".bias"]
        Co = w.shape[0]
        y = conv_rows(src.v, w, B, mesh) + bias
        rec = dict(conv=conv, bn=bn, src=src, dst=dst, col=col, act=act, res=res, y=y)
        if bn is None:
            z = y
        else:
            mean, var = y.mean(0), y.var(0, unbiased=False)
            rstd = 1.0 / torch.sqrt(var + EPS)
            a = sd[bn + ".weight"] * rstd
            b = sd[bn + ".bias"] - mean * a
            z = y * a + b
            stats[bn + ".running_mean"] = (1 - MOMENTUM) * sd[bn + ".running_mean"] + MOMENTUM * mean
            stats[bn + ".running_var"] = (1 - MOMENTUM) * sd[bn + ".running_var"] + MOMENTUM * var * M / (M - 1)
            stats[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + 1
            rec.update(mean=mean, rstd=rstd, a=a)
        rec["z"] = z
        v = torch.where(z > 0, z, 0.2 * z) if act else z
        if res is not None:
            v = v + res.v
        if dst is not None:
            dst.v[:, col:col + Co] = v
        tape.append(rec)
        return v

    def block(q, src, dst, col=0):
        return layer(q + ".convolution", q + ".batch_norm", src, dst, col)

    def res_block(i, xb, width):
        q = f"res_nets.{i}"
        hb, yb = _Buf(M, width), _Buf(M, width)
        layer(q + ".convolution1", q + ".batch_norm1", xb, hb)
        layer(q + ".convolution2", q + ".batch_norm2", hb, yb, act=False, res=xb)
        return yb

    p0 = _Buf(M, C)
    p0.v[:] = x.reshape(M, C)
    p1 = _Buf(M, 64)
    layer("lift.inter_CNOBlock.convolution", None, p0, p1)
    xb = _Buf(M, WIDTHS[0])
    layer("lift.convolution", None, p1, xb, act=False)
    skip = []
    for i in range(3):
        skip.append(res_block(i, xb, WIDTHS[i]))
        nb = _Buf(M, WIDTHS[i + 1])
        block(f"encoder.{i}", xb, nb)
        xb = nb
    for j in range(6):                                                # res_nets[-1], res_nets[-2], ... res_nets[-6]
        xb = res_block(8 - j, xb, 128)
    a = _Buf(M, 128)
    block("ED_expansion.3", xb, a)
    b = _Buf(M, 128)
    block("decoder_inv.0", a, b)
    c1 = _Buf(M, 128)
    block("decoder.0", b, c1, 0)
    block("ED_expansion.2", skip[2], c1, 64)
    b = _Buf(M, 128)
    block("decoder_inv.1", c1, b)
    c2 = _Buf(M, 64)
    block("decoder.1", b, c2, 0)
    block("ED_expansion.1", skip[1], c2, 32)
    b = _Buf(M, 64)
    block("decoder_inv.2", c2, b)
    c3 = _Buf(M, 32)
    block("decoder.2", b, c3, 0)
    block("ED_expansion.0", skip[0], c3, 16)
    d = _Buf(M, 64)
    layer("project.inter_CNOBlock.convolution", None, c3, d)
    out_rows = layer("project.convolution", None, d, act=False)
    out = out_rows.reshape(B, T, H, W, -1).reshape(target.shape)
    loss = ((out - target) ** 2).mean()

    # ---------------------------------------------------------------- backward: the tape in reverse
    g = {}                                                            # id(buffer) -> gradient [M][width]
    g_out = (2.0 / out.numel()) * (out - target).reshape(M, -1)
    for rec in reversed(tape):
        conv, bn, src, dst, col = rec["conv"], rec["bn"], rec["src"], rec["dst"], rec["col"]
        w = sd[conv + ".weight"]
        Co = w.shape[0]
        gv = g_out if dst is None else g[id(dst)][:, col:col + Co]
        if rec["res"] is not None:                                    # the residual passes gv on unchanged
            k = id(rec["res"])
            g[k] = g[k] + gv if k in g else gv.clone()
        dz = torch.where(rec["z"] > 0, gv, 0.2 * gv) if rec["act"] else gv
        if bn is None:
            dy = dz
        else:
            xhat = (rec["y"] - rec["mean"]) * rec["rstd"]
            dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
            dy = rec["a"] * (dz - dbeta / M - xhat * dgamma / M)
            grads[bn + ".weight"], grads[bn + ".bias"] = dgamma, dbeta
        grads[conv + ".weight"], grads[conv + ".bias"] = weight_grad(dy, src.v, B, mesh), dy.sum(0)
        if src is not p0:                                             # lift.0 needs no data gradient
            dx = conv_rows(dy, flipped(w), B, mesh)
            g[id(src)] = g[id(src)] + dx if id(src) in g else dx
    return out, loss, stats, grads
