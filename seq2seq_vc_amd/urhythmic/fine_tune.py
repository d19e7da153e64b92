"""The vocoder fine-tuning step of the reference (urhythmic_fine_tune_vocoder.py:191-222) as one object over this package's pieces: the
trainable HifiganGenerator, the HifiganDiscriminator, LogMelSpectrogram.l1_loss, the three GAN losses of urhythmic/vocoder.py and
optim.MultiAdamW.

    tuner = VocoderFineTuner(generator, discriminator)            # the reference script's constants (:39-46) are the defaults
    for wavs, units, tgts in loader:
        losses = tuner.step(wavs, units, tgts)                    # three 0-dim device tensors, no host read
    tuner.end_epoch()                                             # both ExponentialLR schedulers

mode="reference" is the loop body in the reference's order with its quirks: the generator half calls D(wavs) and D(wavs_) under grad
mode, so loss_generator.backward() computes every discriminator weight gradient of both calls and ADDS them to the .grad the
discriminator half left -- sums that the next step's zero_grad() discards unread.
mode="lean" (the default) is the same step, except that in the generator half D(wavs) runs under no_grad and D(wavs_) runs while the
discriminator's parameters do not require grad (restored afterwards, also on an exception): the backward then executes
backward_plan(need_dx=True, need_params=False) for the generated branch and nothing at all for the real one.  Every power iteration
of the spectrally normed scale still happens (four per step in train() mode).  The updated parameters, both optimiser states, the
weight_u / weight_v buffers and the three losses have the same bits in both modes; the ONLY observable difference is what the
discriminator's .grad holds after the step (lean: the gradients of the discriminator loss that its optimiser consumed).

`launch_plan()` lists the library launches of one step per stage: the concatenation of what the nets themselves say a forward or a
backward of theirs calls (`HifiganGenerator.calls`, `HifiganDiscriminator.calls`; vocoder/plan.py) under this step's stage labels,
plus the loss and optimiser launches of its own; step() executes exactly that list.  What is still ATen inside a
step, in both modes: the scalar combination 45 loss_mel + 2 loss_features + loss_adversarial with its backward, autograd's sums of the
data gradients that meet at wavs_ (and at the pooled inputs of the scales), and -- in reference mode only -- the accumulation into
the discriminator's .grad.  Out of scope: graph capture of the step, DDP, one B = 16 discriminator call for real and generated (it
halves the power iterations per step and so changes the trajectory), bf16 discriminators, MelDataset."""
import contextlib

import torch

from ..ops import functional as Fn
from ..ops import kernels_ganloss as KG
from ..optim import MultiAdamW
from ..vocoder.hifigan import HifiganGenerator
from .dataset import LogMelSpectrogram
from .vocoder import HifiganDiscriminator, discriminator_loss, feature_loss, generator_loss

MODES = ("lean", "reference")
MEL_WEIGHT, FEATURE_WEIGHT = 45, 2


class VocoderFineTuner:
    """One fine-tuning step of the HiFi-GAN vocoder (module docstring).  generator: this package's HifiganGenerator (switched to
    trainable()); discriminator: this package's HifiganDiscriminator; melspectrogram: this package's LogMelSpectrogram (None: the
    default one, on the generator's device).  Anything else raises.  The optimisers are MultiAdamW, the schedulers ExponentialLR;
    `optimizer_generator`, `optimizer_discriminator`, `scheduler_generator`, `scheduler_discriminator` are public."""

    def __init__(self, generator, discriminator, melspectrogram=None, lr=5e-5, betas=(0.8, 0.99), weight_decay=1e-2, lr_decay=0.999,
                 mode="lean"):
        if not isinstance(generator, HifiganGenerator):
            raise TypeError(f"VocoderFineTuner: generator must be seq2seq_vc_amd.vocoder.HifiganGenerator, got {type(generator).__name__}")
        if not isinstance(discriminator, HifiganDiscriminator):
            raise TypeError("VocoderFineTuner: discriminator must be seq2seq_vc_amd.urhythmic.vocoder.HifiganDiscriminator, got "
                            f"{type(discriminator).__name__}")
        if mode not in MODES:
            raise ValueError(f"VocoderFineTuner: mode is one of {MODES}")
        device = next(generator.parameters()).device
        if melspectrogram is None:
            melspectrogram = LogMelSpectrogram().to(device)
        if not isinstance(melspectrogram, LogMelSpectrogram):
            raise TypeError("VocoderFineTuner: melspectrogram must be seq2seq_vc_amd.urhythmic.dataset.LogMelSpectrogram, got "
                            f"{type(melspectrogram).__name__}")
        if any(not leaf.normed for _, leaf in generator._leaves()):
            raise ValueError("VocoderFineTuner: the generator is fine-tuned in its weight-norm form (weight_g, weight_v)")
        self.generator, self.discriminator, self.melspectrogram, self.mode = generator.trainable(), discriminator, melspectrogram, mode
        self.generator.train()
        self.discriminator.train()
        self.optimizer_generator = MultiAdamW(generator.parameters(), lr=lr, betas=betas, weight_decay=weight_decay)
        self.optimizer_discriminator = MultiAdamW(discriminator.parameters(), lr=lr, betas=betas, weight_decay=weight_decay)
        self.scheduler_generator = torch.optim.lr_scheduler.ExponentialLR(self.optimizer_generator, gamma=lr_decay)
        self.scheduler_discriminator = torch.optim.lr_scheduler.ExponentialLR(self.optimizer_discriminator, gamma=lr_decay)

    # ---- the launch list ----------------------------------------------------------------------------------------------------
    def launch_plan(self):
        """The library launches of one step(), in order, one dict per call into the library: `stage`, `call` (the entry point's name
        without the prefix) and the fields of the net's own plan entry it came from.  step() executes exactly this list (within one
        backward stage the order of the sub-discriminators' nodes is autograd's: the last one made first)."""
        G, D, lean = self.generator, self.discriminator, self.mode == "lean"

        def own(stage, *calls):
            return [dict(stage=stage, kind="loss" if "loss" in c else "optimizer", call=c) for c in calls]

        plan = G.calls(G.train_plan(torch.float32), "generator forward")
        plan += D.calls("discriminator half: D(wavs)")
        plan += D.calls("discriminator half: D(wavs_.detach())")
        plan += own("discriminator half: discriminator_loss", "gan_score_loss")
        plan += own("discriminator half: backward", "gan_score_loss_bwd")
        plan += D.calls("discriminator half: backward of D(wavs_.detach())", (False, True))
        plan += D.calls("discriminator half: backward of D(wavs)", (False, True))
        plan += own("discriminator half: optimizer_discriminator.step", *["adamw_multi"] * self.optimizer_discriminator.launches_per_step())
        plan += D.calls("generator half: D(wavs)" + (" under no_grad" if lean else ""))
        plan += D.calls("generator half: D(wavs_)" + (" with frozen parameters" if lean else ""))
        plan += own("generator half: mel l1_loss", "melspec_fwd", "melspec_loss_finish")
        plan += own("generator half: feature_loss", "gan_feature_loss")
        plan += own("generator half: generator_loss", "gan_score_loss")
        plan += own("generator half: backward", "gan_score_loss_bwd", "gan_feature_loss_bwd", "melspec_bwd_frames", "melspec_bwd_ola")
        plan += D.calls("generator half: backward of D(wavs_)", (True, not lean))
        if not lean:
            plan += D.calls("generator half: backward of D(wavs)", (False, True))
        plan += G.calls(G.backward_plan(), "generator half: backward of the generator")
        plan += own("generator half: optimizer_generator.step", *["adamw_multi"] * self.optimizer_generator.launches_per_step())
        return plan

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _check_batch(self, **tensors):
        for name, t in tensors.items():
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"VocoderFineTuner: {name} must be a tensor")
            if t.dtype in (torch.bfloat16, torch.float16):
                raise NotImplementedError(f"VocoderFineTuner runs in fp32 only ({name} is {t.dtype}): a 16-bit discriminator forward flips "
                                          "leaky-relu masks (DESIGN.md section 8)")
            if t.dtype != torch.float32:
                raise TypeError(f"VocoderFineTuner: float32 {name}")
            if not t.is_cuda:
                raise RuntimeError(f"VocoderFineTuner needs GPU tensors ({name} is on the CPU; there is no CPU path)")
        if Fn.compute_dtype() != torch.float32:
            raise NotImplementedError("VocoderFineTuner runs under the fp32 compute dtype only")

    @contextlib.contextmanager
    def _frozen_discriminator(self):
        params = [p for p in self.discriminator.parameters() if p.requires_grad]
        try:
            for p in params:
                p.requires_grad_(False)
            yield
        finally:
            for p in params:
                p.requires_grad_(True)

    def step(self, wavs, units, tgts):
        """One step on a batch (wavs (B, 1, T), units (B, in_channels, N), tgts of melspectrogram.output_shape(wavs.shape)) ->
        {"loss_mel", "loss_discriminator", "loss_generator"}: detached 0-dim device tensors; nothing is read back to the host."""
        self._check_batch(wavs=wavs, units=units, tgts=tgts)
        G, D, lean = self.generator, self.discriminator, self.mode == "lean"
        # Discriminator
        self.optimizer_discriminator.zero_grad()
        wavs_ = G(units)
        scores, _ = D(wavs)
        scores_, _ = D(wavs_.detach())
        loss_discriminator, _, _ = discriminator_loss(scores, scores_, detail=False)
        loss_discriminator.backward()
        self.optimizer_discriminator.step()
        # Generator
        self.optimizer_generator.zero_grad()
        if lean:
            with torch.no_grad():
                _, features = D(wavs)
            with self._frozen_discriminator():
                scores_, features_ = D(wavs_)
        else:
            _, features = D(wavs)
            scores_, features_ = D(wavs_)
        loss_mel, _ = self.melspectrogram.l1_loss(wavs_, tgts)
        loss_features = feature_loss(features, features_)
        loss_adversarial, _ = generator_loss(scores_)
        loss_generator = MEL_WEIGHT * loss_mel + FEATURE_WEIGHT * loss_features + loss_adversarial
        loss_generator.backward()
        self.optimizer_generator.step()
        return {"loss_mel": loss_mel.detach(), "loss_discriminator": loss_discriminator.detach(), "loss_generator": loss_generator.detach()}

    def validate(self, wavs, units, tgts):
        """The reference's validation loss (:258-264): under no_grad, the L1 distance of the generated log-mel and tgts on their
        common length -> a 0-dim device tensor.  (wavs is taken for the loop's call shape and not read.)"""
        self._check_batch(units=units, tgts=tgts)
        with torch.no_grad():
            mels_ = self.melspectrogram(self.generator(units))
            length = min(mels_.size(-1), tgts.size(-1))
            a, b = mels_[..., :length].contiguous(), tgts[..., :length].contiguous()
            if a.shape != b.shape:
                raise ValueError(f"validate: log-mel {tuple(mels_.shape)} against targets {tuple(tgts.shape)}")
            return KG.feature_loss_fwd([(a, b)])[0]

    def end_epoch(self):
        self.scheduler_generator.step()
        self.scheduler_discriminator.step()

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------
    def checkpoint(self, step, loss):
        """The dict the reference's loop saves: {"generator": {"model", "optimizer", "scheduler"}, "discriminator": {...}, "step",
        "loss"}.  Every tensor is a copy: the dict does not move with later steps."""
        def block(model, optimizer, scheduler):
            return {"model": {k: v.detach().clone() for k, v in model.state_dict().items()}, "optimizer": optimizer.state_dict(),
                    "scheduler": dict(scheduler.state_dict())}
        return {"generator": block(self.generator, self.optimizer_generator, self.scheduler_generator),
                "discriminator": block(self.discriminator, self.optimizer_discriminator, self.scheduler_discriminator),
                "step": step, "loss": loss}

    def load_checkpoint(self, state, finetune=False):
        """-> (step, loss).  finetune=True loads the two models alone and returns (0, inf): a pre-trained vocoder starts its
        fine-tuning with fresh optimisers and schedulers, as the reference's loader does."""
        self.generator.load_state_dict(state["generator"]["model"])
        self.discriminator.load_state_dict(state["discriminator"]["model"])
        if finetune:
            return 0, float("inf")
        self.optimizer_generator.load_state_dict(state["generator"]["optimizer"])
        self.scheduler_generator.load_state_dict(state["generator"]["scheduler"])
        self.optimizer_discriminator.load_state_dict(state["discriminator"]["optimizer"])
        self.scheduler_discriminator.load_state_dict(state["discriminator"]["scheduler"])
        return state["step"], state["loss"]

