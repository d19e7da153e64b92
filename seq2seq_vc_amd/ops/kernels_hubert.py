"""Launchers of the HuBERT-Soft content encoder's own kernels (csrc/attn_flash.hip, csrc/hubert.hip; C ABI in include/s2svc_hip.h):
attention forward without the map, front-end layer 0 (convolution + per-row GroupNorm + GELU) and the unit log-probs.
Non-differentiable, GPU tensors only; every argument is device-resident, so no launcher waits for the device."""
import torch

from .. import _lib
from .kernels import _need_cuda, dt, ptr, stream

DK = 64                      # head width of the flash kernel
MAX_K = 256                  # label embeddings of the logits kernel (the hub model has 100)
UNIT_DIM = 256
C0 = 512                     # channels of front-end layer 0
PAD = 40                     # zero samples HubertSoft.units puts on both sides of the waveform: (400 - 320) // 2


def frames0(n, pad=PAD):
    """Frames of front-end layer 0 for a waveform of n samples padded by `pad` on both sides."""
    n = int(n) + 2 * pad
    return 0 if n < 10 else (n - 10) // 5 + 1


def _view_ok(t, name):
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{name}: a (B, T, H * dk) view with unit stride in its last dimension expected, got {tuple(t.shape)} {t.stride()}")


def attn_flash_supported(dtype, dk, ldq, ldk, ldv, ldo):
    """True if attn_flash_fwd takes the problem (fp32 / bf16, dk = 64, row strides of whole 16-byte vectors)."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return bool(_lib.lib().s2svc_attn_flash_supported(dt(dtype), int(dk), int(ldq), int(ldk), int(ldv), int(ldo)))


def attn_flash_fwd(q, k, v, H, klen=None, scale=None, out=None):
    """q (B, T1, H * 64), k / v (B, T2, H * 64): views with any batch and row strides (slices of a packed (B, T, 3 D) projection),
    klen (B) int32 or None -> ctx (B, T1, H * 64) = softmax(scale q k^T) v per head, without the attention map.  Keys at or beyond
    klen[b] are never read; query rows at or beyond klen[b] are +0.  out: a view to write into (only its (B, T1, H * 64) elements are
    written).  One launch."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _view_ok(t, n)
    _need_cuda(q, k, v, klen, out)
    B, T1, D = q.shape
    T2 = k.shape[1]
    if D != H * DK or k.shape != (B, T2, D) or v.shape != (B, T2, D) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"attn_flash_fwd: q (B, T1, {H} * {DK}) and k, v (B, T2, {H} * {DK}) of one dtype expected, got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    if klen is not None and (klen.dtype != torch.int32 or not klen.is_contiguous() or klen.numel() != B):
        raise ValueError(f"klen: a contiguous int32 tensor of {B} values expected")
    if out is None:
        out = torch.empty(B, T1, D, dtype=q.dtype, device=q.device)
    else:
        _view_ok(out, "out")
        if out.shape != (B, T1, D) or out.dtype != q.dtype:
            raise ValueError("attn_flash_fwd: out must be a (B, T1, H * dk) view of the input dtype")
    if not attn_flash_supported(q.dtype, DK, q.stride(1), k.stride(1), v.stride(1), out.stride(1)):
        raise NotImplementedError(f"attn_flash_fwd: unsupported problem (dtype {q.dtype}, row strides {q.stride(1)}, {k.stride(1)}, "
                                  f"{v.stride(1)}, {out.stride(1)}): there is no other path")
    scale = DK ** -0.5 if scale is None else float(scale)
    _lib.check(_lib.lib().s2svc_attn_flash_fwd(dt(q), B, H, T1, T2, DK, ptr(q), q.stride(0), q.stride(1), ptr(k), k.stride(0), k.stride(1),
                                               ptr(v), v.stride(0), v.stride(1), ptr(klen), scale, ptr(out), out.stride(0), out.stride(1),
                                               stream()), "attn_flash_fwd")
    return out


def _conv0_args(wav, lens, w):
    if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_contiguous():
        raise ValueError(f"wav: contiguous fp32 (B, Nmax) expected, got {wav.dtype} {tuple(wav.shape)}")
    B = wav.shape[0]
    if lens.dtype != torch.int32 or not lens.is_contiguous() or lens.numel() != B:
        raise ValueError(f"lens: a contiguous int32 tensor of {B} values expected")
    if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != C0 * 10:
        raise ValueError(f"layer-0 weight: contiguous fp32 ({C0}, 1, 10) expected, got {w.dtype} {tuple(w.shape)}")
    _need_cuda(wav, lens, w)
    return B, wav.shape[1]


def conv0_ws(B, device):
    """The statistics workspace of B rows: 32 ordered chunk pairs of double sums per (row, channel)."""
    return torch.empty(_lib.lib().s2svc_hubert_conv0_ws_bytes(B) // 8, dtype=torch.float64, device=device)


def conv0_stats(wav, lens, w, ws, pad=PAD):
    """wav (B, Nmax) fp32, lens (B) int32, w (512, 1, 10) -> ws: sum y and sum y^2 of every (row, channel) over the row's own frames."""
    B, Nmax = _conv0_args(wav, lens, w)
    _lib.check(_lib.lib().s2svc_hubert_conv0_stats(B, Nmax, int(pad), ptr(wav), ptr(lens), ptr(w), ptr(ws), stream()), "hubert_conv0_stats")
    return ws


def conv0_apply(wav, lens, w, gamma, beta, ws, L0max, out_dtype, eps=1e-5, pad=PAD, out=None):
    """-> (B, L0max, 512) channel-last in out_dtype: GELU(GroupNorm(conv0(wav))) with the statistics of ws; +0 beyond a row's frames."""
    B, Nmax = _conv0_args(wav, lens, w)
    if out is None:
        out = torch.empty(B, int(L0max), C0, dtype=out_dtype, device=wav.device)
    elif out.shape != (B, int(L0max), C0) or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError("conv0_apply: out must be a contiguous (B, L0max, 512) tensor of out_dtype")
    _lib.check(_lib.lib().s2svc_hubert_conv0_apply(dt(out_dtype), B, Nmax, int(pad), int(L0max), ptr(wav), ptr(lens), ptr(w), ptr(gamma),
                                                   ptr(beta), float(eps), ptr(ws), ptr(out), stream()), "hubert_conv0_apply")
    return out


def front_layer0(wav, lens, w, gamma, beta, L0max, out_dtype, eps=1e-5, pad=PAD):
    """The two launches of front-end layer 0."""
    ws = conv0_stats(wav, lens, w, conv0_ws(wav.shape[0], wav.device), pad)
    return conv0_apply(wav, lens, w, gamma, beta, ws, L0max, out_dtype, eps, pad)


def hubert_logits(units, emb, lens=None, log_softmax=True, out=None):
    """units (B, L, 256) fp32 / bf16 contiguous, emb (K <= 256, 256) fp32, lens (B) int32 or None -> (B, L, K) fp32:
    log_softmax(cosine_similarity(units, emb) / 0.1) (log_softmax=False: the quotient, Hubert.logits); rows beyond lens are +0."""
    if units.dim() != 3 or units.shape[2] != UNIT_DIM or not units.is_contiguous():
        raise ValueError(f"units: contiguous (B, L, {UNIT_DIM}) expected, got {tuple(units.shape)}")
    if emb.dim() != 2 or emb.shape[1] != UNIT_DIM or emb.dtype != torch.float32 or not emb.is_contiguous() or not 1 <= emb.shape[0] <= MAX_K:
        raise ValueError(f"label embedding: contiguous fp32 (K <= {MAX_K}, {UNIT_DIM}) expected, got {emb.dtype} {tuple(emb.shape)}")
    B, L, _ = units.shape
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_contiguous() or lens.numel() != B):
        raise ValueError(f"lens: a contiguous int32 tensor of {B} values expected")
    _need_cuda(units, emb, lens)
    K = emb.shape[0]
    if out is None:
        out = torch.empty(B, L, K, dtype=torch.float32, device=units.device)
    elif out.shape != (B, L, K) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("hubert_logits: out must be a contiguous fp32 (B, L, K) tensor")
    if B * L == 0:
        return out
    _lib.check(_lib.lib().s2svc_hubert_logits(dt(units), B, L, K, 1 if log_softmax else 0, ptr(units), ptr(lens), ptr(emb), ptr(out),
                                              stream()), "hubert_logits")
    return out
