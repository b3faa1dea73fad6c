"""Plain float64 reference of one SRU layer on the CPU: the formulas of the SRU class's contract, literally, with a Python
loop over t; gradients come from autograd."""
import torch

SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
ACTS = {"none": lambda c: c, "tanh": torch.tanh, "relu": torch.relu,
        "selu": lambda c: SELU_SCALE * torch.where(c > 0, c, SELU_ALPHA * (torch.exp(c) - 1.0))}


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def sru_scan_ref(U, x_skip, weight_c, bias, scale_x, act, D, mask_h=None, cs=None):
    """U [T, B, out * k] -> Y [T, B, out]; cs (a list) collects every c_t."""
    T, B, W = U.shape
    out = weight_c.numel() // 2
    H, k = out // D, W // out
    u = U.reshape(T, B, out, k)
    vf, vr, bf, br = weight_c[:out], weight_c[out:], bias[:out], bias[out:]
    rev = (torch.arange(out) >= H) if D == 2 else torch.zeros(out, dtype=torch.bool)
    c = U.new_zeros(B, out)
    hs = [None] * T
    for s in range(T):
        # direction 0 is at time s, direction 1 at time T - 1 - s
        us = torch.where(rev[None, :, None], u[T - 1 - s], u[s])
        f = torch.sigmoid(us[..., 1] + vf * c + bf)
        r = torch.sigmoid(us[..., 2] + vr * c + br)
        c = us[..., 0] + (c - us[..., 0]) * f
        if cs is not None:
            cs.append(c)
        g = ACTS[act](c) * (mask_h if mask_h is not None else 1.0)
        if k == 4:
            xp = us[..., 3]
        elif x_skip is not None:
            xp = scale_x * torch.where(rev[None, :], x_skip[T - 1 - s], x_skip[s])
        else:
            xp = torch.zeros_like(c)
        hs[s] = xp + (g - xp) * r
    return torch.stack([torch.where(rev[None, :], hs[T - 1 - t], hs[t]) for t in range(T)])


def sru_layer_ref(x, cell, k, skip, scale_x, act, D, m_rnn=None, m_h=None, bf16_operands=False, cs=None):
    """One layer from its parameters (cell: dict weight / weight_proj / weight_c / bias).  bf16_operands: every GEMM operand
    takes its bf16 value (forward: x~, x~ . weight_proj and both weights, as constants of the rounding; backward: the
    gradient of each product, the operand of the dX / dW products)."""
    rnd = (lambda t: t + (bf16(t.detach()) - t.detach())) if bf16_operands else (lambda t: t)

    def product(a, w):
        p = a @ rnd(w)
        if bf16_operands and p.requires_grad:
            p.register_hook(bf16)
        return p

    z = rnd(x * m_rnn if m_rnn is not None else x)
    if cell.get("weight_proj") is not None:
        z = rnd(product(z, cell["weight_proj"]))
    U = product(z, cell["weight"])
    return sru_scan_ref(U, x if skip else None, cell["weight_c"], cell["bias"], scale_x, act, D, m_h, cs)
