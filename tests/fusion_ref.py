"""Plain float64 reference of the fusion layer and of the fusionRNN_jit stack on the CPU: the formulas of the class's
contract, literally, with a Python loop over t; gradients come from autograd.  bf16_operands: every GEMM operand takes its
bf16 value where the engine's bf16 mode rounds it - x and W of a projection, h and U of the recurrence, and in backward the
gradient of each product (the operand of the dX / dW products), the gradient the fusion layer receives and, on the layers
the engine runs on its perf node, the gate gradients in front of the BatchNorm backward (see fusion_rnn_ref)."""
import torch


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _product(a, w, on):
    """a . w^T; with `on`, both operands as constants of the rounding and the product's gradient rounded."""
    if not on:
        return a @ w.t()
    p = (a + (bf16(a.detach()) - a.detach())) @ (w + (bf16(w.detach()) - w.detach())).t()
    if p.requires_grad:
        p.register_hook(bf16)
    return p


def fusion_proj_ref(x, W, b, slope, M, act, reduce, bf16_operands=False, pres=None):
    """x [N, M*F], W [2*H0, F], b [2*H0], slope [2] or None -> P [N, 2*H0]; pres (a list) collects the pre-activations."""
    N, F, H0 = x.shape[0], W.shape[1], W.shape[0] // 2
    pre = _product(x.reshape(N * M, F), W, bf16_operands).reshape(N, M, 2 * H0) + b
    if pres is not None:
        pres.append(pre.detach())
    if act == "prelu":
        a = torch.where(pre > 0, pre, torch.cat([slope[:1].expand(H0), slope[1:].expand(H0)]) * pre)
    elif act == "leaky_relu":
        a = torch.where(pre > 0, pre, 0.01 * pre)
    else:
        a = torch.relu(pre) if act == "relu" else torch.tanh(pre)
    out = a.mean(1) if reduce == "mean" else a.sum(1)
    if bf16_operands and out.requires_grad:
        out.register_hook(bf16)
    return out


def fusion_rnn_ref(sd, x, M, act, reduce, masks, training, bf16_operands=False, kinks=None):
    """The whole class from a state dict of float64 tensors (running statistics are updated in place in training mode).
    masks: per layer [2B, H_i] or None (the scalar 1.0).  kinks (a list) collects |.| of every piecewise-linear
    pre-activation: the fusion layer's and the recurrences' ReLU candidates."""
    T, B, _ = x.shape
    L = 1 + max(int(k.split(".")[1]) for k in sd)
    for i in range(L):
        g = lambda n: sd["model.%d.%s" % (i, n)]  # noqa: E731
        if i == 0:
            H = g("wz.conv.bias").numel()
            W = torch.cat([g("wz.conv.weight").reshape(H, -1), g("wh.conv.weight").reshape(H, -1)])
            slope = torch.cat([g("wz.act_function.weight"), g("wh.act_function.weight")]) if act == "prelu" else None
            pres = []
            P = fusion_proj_ref(x.reshape(T * B, -1), W, torch.cat([g("wz.conv.bias"), g("wh.conv.bias")]), slope, M, act, reduce,
                                bf16_operands, pres)
            if kinks is not None and act != "tanh":
                kinks.append(pres[0].abs())
        else:
            H = g("wz.bias").numel()
            P = _product(x.reshape(T * B, -1), torch.cat([g("wz.weight"), g("wh.weight")]), bf16_operands)
            P = P + torch.cat([g("wz.bias"), g("wh.bias")])
        P = P.reshape(T, B, 2 * H)
        P = torch.cat([P, P.flip(0)], 1).reshape(2 * T * B, 2 * H)  # the reference's cat([x, flip(x)], dim=1), projected
        n = P.shape[0]
        halves = []
        for k, name in enumerate(("bn_wz", "bn_wh")):
            p = P[:, k * H:(k + 1) * H]
            if training:
                mean, var = p.mean(0), p.var(0, unbiased=False)
                with torch.no_grad():
                    g(name + ".running_mean").mul_(0.95).add_(0.05 * mean)
                    g(name + ".running_var").mul_(0.95).add_(0.05 * var * n / (n - 1))
                    g(name + ".num_batches_tracked").add_(1)
            else:
                mean, var = g(name + ".running_mean"), g(name + ".running_var")
            halves.append((p - mean) / torch.sqrt(var + 1e-5) * g(name + ".weight") + g(name + ".bias"))
        wz, wh = (h.reshape(T, 2 * B, H) for h in halves)
        if bf16_operands and training and i > 0 and wz.requires_grad:
            # layers 1 and up in bf16 training run on the engine's perf node (functional.RecLayerPerfFn), where "the fp32
            # gate-gradient slabs never exist": BatchNorm backward reads the gate gradients as the bf16 operands of the
            # carry / dU products.  Layer 0 and every eval-mode layer run on the general node, which keeps them in fp32.
            wz.register_hook(bf16)
            wh.register_hook(bf16)
        m = masks[i] if masks is not None and masks[i] is not None else 1.0
        h = x.new_zeros(2 * B, H)
        hs = []
        for t in range(T):
            uz, uh = _product(h, g("u.weight"), bf16_operands).chunk(2, 1)
            z = torch.sigmoid(wz[t] + uz)
            a = wh[t] + uh
            if kinks is not None:
                kinks.append(a.detach().abs())
            h = z * h + (1 - z) * (torch.relu(a) * m)
            hs.append(h)
        hs = torch.stack(hs)
        x = torch.cat([hs[:, :B], hs[:, B:].flip(0)], 2)
    return x
