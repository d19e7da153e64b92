"""HuBERT-Soft content encoder on HIP (inference): waveform -> soft speech units, the model the reference's urhythmic scripts fetch with
torch.hub.load("bshall/hubert:main", "hubert_soft") and hand to urhythmic/model.py:encode.  Same constructor, methods and state_dict keys
and shapes as upstream's Hubert / HubertSoft, so a locally saved hub checkpoint loads with load_state_dict.

What runs where (csrc/, launchers in ops/kernels_hubert.py):
  front-end layer 0      hubert.hip: statistics launch + apply launch (convolution, per-row GroupNorm, GELU), channel-last output
  feature convs 1 - 6    one batched dense GEMM each: in channel-last storage output frame t reads the contiguous span
                         [s t C, s t C + k C), so A has ld = s C and K = k C against the tap-major weight (O, tap C + c); GELU epilogue
  feature projection     LayerNorm launch + GEMM
  positional conv        16 conv-mode GEMMs (one per group: C = width / 16 channels, 128 taps, pad 64) with bias, GELU and the
                         residual in the epilogue; the weight-norm fold (dim = 2: one norm per tap) is a derived weight
  12 post-LN layers      packed Q|K|V GEMM, attn_flash.hip (no attention map), out-projection GEMM, residual + LayerNorm, two GEMMs of
                         the feed-forward block, residual + LayerNorm: 7 launches a layer
  proj, logits           GEMM; hubert.hip: cosine similarity against the label embedding / 0.1 (and log_softmax for encode())
Derived weights (tap-major convolution weights, the folded positional weight, compute-dtype casts) are made once and remade when a
parameter's version, dtype or device changes, or the compute dtype (ops.functional.set_compute_dtype) does.

Scope: inference.  Masking and dropout act only while training upstream; a module in train() mode, a call that records gradients or
a CPU tensor raises NotImplementedError.  Utterances of more than 4096 frames (the segmenter's limit) are refused."""
import torch
from torch import nn

from ..ops import functional as Fn
from ..ops import kernels as K
from ..ops import kernels_hubert as KH
from ..ops import kernels_sdp as KS

MAX_FRAMES = 4096
_CONVS = ((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2))        # (kernel, stride) of feature_extractor.conv0 .. conv6


def frame_count(n):
    """Frames the feature extractor makes of n samples (HubertSoft.units: the waveform's samples + 80): 400 -> 1, then one per 320."""
    n = int(n)
    for k, s in _CONVS:
        n = (n - k) // s + 1 if n >= k else 0
    return n


class _FeatureExtractor(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv0 = nn.Conv1d(1, 512, 10, 5, bias=False)
        self.norm0 = nn.GroupNorm(512, 512)
        for i, (k, s) in enumerate(_CONVS[1:], 1):
            setattr(self, f"conv{i}", nn.Conv1d(512, 512, k, s, bias=False))


class _FeatureProjection(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.norm = nn.LayerNorm(512)
        self.projection = nn.Linear(512, width)


class _WeightNormConv(nn.Module):
    """The parameters of weight_norm(Conv1d(width, width, 128, padding=64, groups=16), dim=2): weight = g v / |v|, one norm per tap."""

    def __init__(self, width):
        super().__init__()
        conv = nn.Conv1d(width, width, 128, padding=64, groups=16)
        self.bias = nn.Parameter(conv.bias.detach().clone())
        self.weight_v = nn.Parameter(conv.weight.detach().clone())
        self.weight_g = nn.Parameter(conv.weight.detach().pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


class _PositionalConvEmbedding(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.conv = _WeightNormConv(width)


class _SelfAttention(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class _EncoderLayer(nn.Module):
    """The parameters of nn.TransformerEncoderLayer(width, heads, ffn, activation="gelu", batch_first=True) (post-LN, eps 1e-5)."""

    def __init__(self, width, ffn):
        super().__init__()
        self.self_attn = _SelfAttention(width)
        self.linear1 = nn.Linear(width, ffn)
        self.linear2 = nn.Linear(ffn, width)
        self.norm1 = nn.LayerNorm(width)
        self.norm2 = nn.LayerNorm(width)


class _TransformerEncoder(nn.Module):
    def __init__(self, width, ffn, layers):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderLayer(width, ffn) for _ in range(layers)])


def _inference_only(module, *tensors, grad_ok=False):
    if module.training:
        raise NotImplementedError("Hubert on HIP is inference only (masking, dropout and the backward pass are not built): call .eval()")
    if not grad_ok and torch.is_grad_enabled():
        raise NotImplementedError("Hubert on HIP records no gradients: call it under torch.no_grad() or torch.inference_mode()")
    for t in tensors:
        if not t.is_cuda:
            raise NotImplementedError("Hubert on HIP needs GPU tensors (there is no CPU path)")


class Hubert(nn.Module):
    def __init__(self, num_label_embeddings: int = 100, mask: bool = True, *, _width: int = 768, _heads: int = 12, _ffn: int = 3072,
                 _layers: int = 12):
        super().__init__()
        if _width != _heads * KH.DK or _width % 16:
            raise ValueError(f"Hubert: the attention kernel needs a head width of {KH.DK} (width = heads * {KH.DK}) and 16 groups divide the width")
        if not 1 <= num_label_embeddings <= KH.MAX_K:
            raise ValueError(f"Hubert: 1 .. {KH.MAX_K} label embeddings")
        self._mask = mask
        self._heads = _heads
        self.feature_extractor = _FeatureExtractor()
        self.feature_projection = _FeatureProjection(_width)
        self.positional_embedding = _PositionalConvEmbedding(_width)
        self.norm = nn.LayerNorm(_width)
        self.encoder = _TransformerEncoder(_width, _ffn, _layers)
        self.proj = nn.Linear(_width, KH.UNIT_DIM)
        self.masked_spec_embed = nn.Parameter(torch.empty(_width).uniform_())
        self.label_embedding = nn.Embedding(num_label_embeddings, KH.UNIT_DIM)
        self._derived_state = None
        self._derived = {}

    # ---- derived weights ---------------------------------------------------------------------------------------------------
    def _cast_params(self):
        """The parameters whose compute-dtype copy a GEMM reads (everything else stays fp32)."""
        ps = [self.feature_projection.projection.weight, self.proj.weight]
        for l in self.encoder.layers:
            ps += [l.self_attn.in_proj_weight, l.self_attn.out_proj.weight, l.linear1.weight, l.linear2.weight]
        return ps

    def fold_positional_weight(self):
        """weight_norm(dim=2): g v / |v| with |v| over (out, in) per tap -> (width, width / 16, 128) fp32."""
        c = self.positional_embedding.conv
        return c.weight_v * (c.weight_g / c.weight_v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())

    def derived(self, dtype=None):
        """The derived weights for the compute dtype, remade only when a parameter's version, dtype or device (or the compute dtype)
        changed since they were made: conv1 .. conv6 tap-major (O, tap * C + c), the folded positional weight tap-major per group
        (width, tap * C + c), and for bf16 the casts of the GEMM weights (the `_s2s_bf16` copies ops.functional reads)."""
        dtype = Fn.compute_dtype() if dtype is None else dtype
        state = (dtype,) + tuple((p._version, p.dtype, p.device) for p in self.parameters())
        if state == self._derived_state:
            return self._derived
        for p in self.parameters():
            if p.dtype != torch.float32:
                raise NotImplementedError(f"Hubert on HIP keeps fp32 parameters (the compute dtype is set by ops.functional.set_compute_dtype), got {p.dtype}")
        with torch.no_grad():
            d = {}
            fe = self.feature_extractor
            for i in range(1, 7):
                w = getattr(fe, f"conv{i}").weight                                   # (O, C, k)
                d[f"conv{i}"] = w.permute(0, 2, 1).reshape(w.shape[0], -1).to(dtype).contiguous()
            w = self.fold_positional_weight()                                        # (width, C, 128)
            d["pos"] = w.permute(0, 2, 1).reshape(w.shape[0], -1).to(dtype).contiguous()
            for p in self._cast_params():
                if dtype == torch.float32:
                    if hasattr(p, "_s2s_bf16"):
                        del p._s2s_bf16
                else:
                    p._s2s_bf16 = K.cast(p.detach().contiguous(), dtype) if p.is_cuda else p.detach().to(dtype)
        self._derived, self._derived_state = d, state
        return d

    # ---- the network -------------------------------------------------------------------------------------------------------
    def _features(self, wav, lens, pad, batched, layer=None):
        """wav (B, Nmax) fp32 on the GPU, lens: host ints -> x (B, Lmax, width) in the compute dtype, frame_lens (host ints),
        frame_lens on the device (int32; None unless batched)."""
        cd, dev = Fn.compute_dtype(), wav.device
        D = self.derived(cd)
        B, Nmax = wav.shape
        lens = [int(n) for n in lens]
        if len(lens) != B or min(lens) < 0 or max(lens) > Nmax:
            raise ValueError(f"lens: {B} lengths in 0 .. {Nmax} expected, got {lens}")
        frame_lens = [frame_count(n + 2 * pad) for n in lens]
        if max(frame_lens) < 1:
            raise ValueError(f"the waveform is too short: {400 - 2 * pad} samples make the first frame")
        if max(frame_lens) > MAX_FRAMES:
            raise ValueError(f"utterances of more than {MAX_FRAMES} frames are not supported, got {max(frame_lens)}")
        lens_d = torch.tensor(lens, dtype=torch.int32).to(dev)
        fl_d = torch.tensor(frame_lens, dtype=torch.int32).to(dev) if batched else None
        fe = self.feature_extractor
        L = KH.frames0(max(lens), pad)
        x = KH.front_layer0(wav, lens_d, fe.conv0.weight, fe.norm0.weight, fe.norm0.bias, L, cd, fe.norm0.eps, pad)
        C = KH.C0
        for i, (k, s) in enumerate(_CONVS[1:], 1):
            Lo = (L - k) // s + 1
            y = torch.empty(B, Lo, C, dtype=cd, device=dev)
            K.gemm(K.operand(x, s * C, bs0=L * C), K.operand(D[f"conv{i}"], k * C), Lo, C, k * C, y, in_dtype=cd, act="gelu", nb0=B,
                   cbs=(Lo * C, 0))
            x, L = y, Lo
        fp = self.feature_projection
        x = Fn.layer_norm(x, fp.norm.weight, fp.norm.bias, fp.norm.eps)
        x = Fn.linear(x, fp.projection.weight, fp.projection.bias)
        W = x.shape[-1]
        if batched:
            x = KS.mask_rows(x, fl_d)            # the positional convolution mixes 128 frames: nothing beyond a row's end may enter
        pc, Cg = self.positional_embedding.conv, W // 16
        x2, y = x.view(B * L, W), torch.empty(B * L, W, dtype=cd, device=dev)
        for g in range(16):
            K.gemm(K.operand(x2, W, mode=K.CONV1D, C=Cg, T=L, pad=64, offset=g * Cg), K.operand(D["pos"], 128 * Cg, offset=g * Cg * 128 * Cg),
                   B * L, Cg, 128 * Cg, y, in_dtype=cd, bias=pc.bias[g * Cg:(g + 1) * Cg], act="gelu", res=x2[:, g * Cg:], ldr=W, ldc=W,
                   out_offset=g * Cg)
        x = Fn.layer_norm(y.view(B, L, W), self.norm.weight, self.norm.bias, self.norm.eps)
        for l in self.encoder.layers[:layer]:
            a = l.self_attn
            qkv = Fn.linear(x, a.in_proj_weight, a.in_proj_bias)
            ctx = KH.attn_flash_fwd(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], self._heads, fl_d)
            h = Fn.linear(ctx, a.out_proj.weight, a.out_proj.bias)
            x, _ = Fn.add_dropout_layer_norm(x, h, l.norm1.weight, l.norm1.bias, l.norm1.eps)
            h = Fn.ffn_act(x, l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, "gelu")
            x, _ = Fn.add_dropout_layer_norm(x, h, l.norm2.weight, l.norm2.bias, l.norm2.eps)
        return x, frame_lens, fl_d

    def _out(self, x, fl_d):
        """Rows beyond a length zeroed (batched), fp32."""
        if fl_d is not None:
            x = KS.mask_rows(x.contiguous(), fl_d)
        return K.cast(x.contiguous(), torch.float32)

    def launch_plan(self, what="units", batched=False, layer=None, dtype=None):
        """The library launches of one call, in order, by the names the launchers report: what = "encode" (Hubert.encode), "units"
        (HubertSoft.units / units_batch) or "model.encode" (urhythmic.model.encode / encode_batch: units + log-probs)."""
        dtype = Fn.compute_dtype() if dtype is None else dtype
        n = len(self.encoder.layers[:layer])
        plan = ["hubert_conv0_stats", "hubert_conv0_apply"] + ["s2svc_gemm"] * 6 + ["layernorm_fwd", "s2svc_gemm"]
        plan += (["mask_rows"] if batched else []) + ["s2svc_gemm"] * 16 + ["layernorm_fwd"]
        plan += ["s2svc_gemm", "attn_flash_fwd", "s2svc_gemm", "layernorm_fwd", "s2svc_gemm", "s2svc_gemm", "layernorm_fwd"] * n
        if what != "encode":
            plan += ["s2svc_gemm"]
        plan += (["mask_rows"] if batched else []) + (["cast"] if dtype != torch.float32 else [])
        if what == "model.encode":
            plan += ["hubert_logits"]
        return plan

    # ---- upstream's interface ----------------------------------------------------------------------------------------------
    def encode(self, x, layer=None):
        """x (B, 1, N) (taken as it is: HubertSoft.units does the padding) -> ((B, L, width) fp32, None: no mask outside training)."""
        _inference_only(self, x)
        wav = _wav2(x)
        y, _, _ = self._features(wav, [wav.shape[1]] * wav.shape[0], 0, False, layer)
        return self._out(y, None), None

    def logits(self, x):
        """x (B, L, 256) -> (B, L, K): cosine similarity with the label embedding / 0.1."""
        _inference_only(self, x)
        return KH.hubert_logits(x.contiguous(), self.label_embedding.weight, log_softmax=False)

    def forward(self, x):
        x, mask = self.encode(x)
        h = Fn.linear(Fn.to_compute(x), self.proj.weight, self.proj.bias)
        return self.logits(K.cast(h, torch.float32)), mask


def _wav2(wav):
    if wav.dim() != 3 or wav.shape[1] != 1:
        raise ValueError(f"wav: (B, 1, N) expected, got {tuple(wav.shape)}")
    return wav[:, 0].to(torch.float32).contiguous()


class HubertSoft(Hubert):
    """HuBERT-Soft (https://arxiv.org/abs/2111.02392): upstream's HubertSoft() is this class with its default sizes."""

    def __init__(self, *, _width: int = 768, _heads: int = 12, _ffn: int = 3072, _layers: int = 12):
        super().__init__(_width=_width, _heads=_heads, _ffn=_ffn, _layers=_layers)

    def _units(self, wav, lens, batched):
        x, frame_lens, fl_d = self._features(wav, lens, KH.PAD, batched)
        u = Fn.linear(x, self.proj.weight, self.proj.bias)
        return self._out(u, fl_d), frame_lens, fl_d

    @torch.inference_mode()
    def units(self, wav: torch.Tensor) -> torch.Tensor:
        """wav (B, 1, N), every row N samples long -> soft speech units (B, L, 256) fp32, L = frame_count(N + 80)."""
        _inference_only(self, wav, grad_ok=True)
        w = _wav2(wav)
        return self._units(w, [w.shape[1]] * w.shape[0], False)[0]

    @torch.inference_mode()
    def units_batch(self, wavs: torch.Tensor, lens):
        """wavs (B, 1, Nmax), lens (B) samples of every row (list or CPU tensor) -> units (B, Lmax, 256) fp32, zero beyond a row's
        frames, and frame_lens (B) int32 on the CPU, frame_lens[b] = frame_count(lens[b] + 80), computed on the host.  Samples beyond
        lens are never read; every row is computed from its own samples only."""
        _inference_only(self, wavs, grad_ok=True)
        u, frame_lens, _ = self._units(_wav2(wavs), _host_lens(lens), True)
        return u, torch.tensor(frame_lens, dtype=torch.int32)


def _host_lens(lens):
    if isinstance(lens, torch.Tensor):
        if lens.is_cuda:
            raise ValueError("lens: a list or a CPU tensor expected (the frame counts are computed on the host, without a device read)")
        return [int(n) for n in lens.tolist()]
    return [int(n) for n in lens]
