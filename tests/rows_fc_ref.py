"""float64 restatement of the MinkowskiNet head's fc_layer on dense rows (hrnet.py:332-339): a kernel-size-1 convolution with
bias, BatchNorm over the rows of the call, ReLU — forward (training / eval) and the backward with a GIVEN ReLU mask, in plain
torch.  tests/test_cpu_rows_fc.py pins it to nn.Linear + nn.BatchNorm1d + nn.ReLU; the GPU tests take it as their yardstick."""
import torch


def fwd(x, w, b, gamma, beta, running_mean, running_var, eps, momentum, training):
    """Returns a dict: y, a (the pre-activation), z, mean, invstd (the statistics the normalisation used) and the running
    statistics after the call (unchanged in eval).  Everything float64."""
    x, w, b, gamma, beta = (t.double() for t in (x, w, b, gamma, beta))
    rm, rv = running_mean.double(), running_var.double()
    z = x @ w.t() + b
    n = x.shape[0]
    if training:
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var = rm, rv
    invstd = 1 / torch.sqrt(var + eps)
    a = gamma * (z - mean) * invstd + beta
    return {"y": a.clamp_min(0), "a": a, "z": z, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv}


def bwd(dy, mask, x, w, gamma, f, training):
    """Gradients for the upstream dy with the ReLU mask ``mask`` (bool (N, c_out)); ``f`` is fwd()'s dict.  Also returns
    ``scale``: per element of dz the same expression with absolute values of every term — what dx, dw and dbias are measured
    against where the true gradient nearly cancels (``abs_dbias``: the per-column sums behind ``scale_dbias``)."""
    dy, x, w, gamma = (t.double() for t in (dy, x, w, gamma))
    g = dy * mask.double()
    xh = (f["z"] - f["mean"]) * f["invstd"]
    dgamma, dbeta = (g * xh).sum(0), g.sum(0)
    if training:
        dz = gamma * f["invstd"] * (g - g.mean(0) - xh * (g * xh).mean(0))
        adz = gamma.abs() * f["invstd"] * (g.abs() + g.abs().mean(0) + xh.abs() * (g * xh).abs().mean(0))
    else:
        dz = g * gamma * f["invstd"]
        adz = dz.abs()
    return {"dx": dz @ w, "dw": dz.t() @ x, "dbias": dz.sum(0), "dgamma": dgamma, "dbeta": dbeta, "dz": dz,
            "scale_dx": (adz @ w.abs()).max(), "scale_dw": (adz.t() @ x.abs()).max(), "scale_dbias": adz.sum(0).max(),
            "abs_dbias": adz.sum(0)}


def inputs(seed, n, c_in, c_out):
    """The test inputs of one case (float32, CPU): x ~ N(0,1), w ~ N(0,1)/sqrt(c_in), bias ~ 0.1 N, gamma ~ 1 + 0.2 N,
    beta ~ 0.3 N, dy ~ N(0,1), running statistics near (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(n, c_in), "w": r(c_out, c_in) / c_in ** 0.5, "b": 0.1 * r(c_out), "gamma": 1 + 0.2 * r(c_out),
            "beta": 0.3 * r(c_out), "dy": r(n, c_out), "running_mean": 0.1 * r(c_out), "running_var": 1 + 0.1 * r(c_out).abs()}
