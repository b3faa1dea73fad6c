"""Helpers of the length-aware decoding tests (test_seq_len_host.py, test_gpu_seq_len.py): the batch of sentences every
test uses, and a pure-torch construction of what pk_seq_pack_len / pk_seq_join_len compute, written with slices and
torch.flip - no index arithmetic shared with the kernels.  test_seq_len_host.py holds it to the reference's own
cat / flip on each sentence alone; the GPU tests hold the kernels to it with torch.equal."""
import torch

T_MAX, LENS = 7, (7, 1, 4, 7, 2)   # five sentences: two of full length, one of a single frame


def host_pack_len(x, lens):
    """x [T, B, D] -> (out_f, out_r): the padding rows zeroed; every sentence reversed on its own, zeros behind."""
    out_f, out_r = torch.zeros_like(x), torch.zeros_like(x)
    for b, n in enumerate(lens):
        out_f[:n, b] = x[:n, b]
        out_r[:n, b] = torch.flip(x[:n, b], [0])
    return out_f, out_r


def host_join_len(hf, hb, lens):
    """hf, hb [T, B, H] (hb in per-sentence reversed order) -> (y, y_rev) [T, B, 2H], zeros behind every sentence."""
    T, B, H = hf.shape
    y = torch.zeros(T, B, 2 * H, dtype=hf.dtype, device=hf.device)
    y_rev = torch.zeros_like(y)
    for b, n in enumerate(lens):
        y[:n, b, :H] = hf[:n, b]
        y[:n, b, H:] = torch.flip(hb[:n, b], [0])
        y_rev[:n, b] = torch.flip(y[:n, b], [0])
    return y, y_rev


def padded_batch(sentences):
    """[L_b, D] tensors -> the end-padded [T, B, D] batch and the lengths."""
    lens = [int(s.shape[0]) for s in sentences]
    x = torch.zeros(max(lens), len(sentences), sentences[0].shape[1])
    for b, s in enumerate(sentences):
        x[:lens[b], b] = s
    return x, lens
