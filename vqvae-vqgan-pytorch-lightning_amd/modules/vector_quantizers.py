"""Quantizers on the vqk kernels; same classes / ctor signatures / return conventions as the reference's
``vqvae/modules/vector_quantizers.py`` (VectorQuantizer :8-84, EMAVectorQuantizer :87-203,
EntropyVectorQuantizer :277-381, GumbelVectorQuantizer :206-274); ``FSQuantizer`` (finite scalar quantization, no counterpart in
the reference) is the fifth member of the family, ``ResidualVectorQuantizer`` (residual quantization, no counterpart either) the sixth,
``CosineVectorQuantizer`` (the l2-normalised low-dimensional codebook of ViT-VQGAN, no counterpart either) the seventh,
``LFQuantizer`` (lookup-free quantization of MAGVIT-v2: sign bits + an entropy loss, no counterpart either) the eighth,
``GroupedVectorQuantizer`` (product quantization: one small codebook per channel group, no counterpart either) the ninth,
``SimVectorQuantizer`` (SimVQ: a frozen code table behind one learned linear layer, no counterpart either) the tenth,
``BSQuantizer`` (binary spherical quantization of BSQ-ViT: ``LFQuantizer`` on the unit sphere, no counterpart either) the eleventh,
``IBQuantizer`` (index backpropagation: a straight-through estimator on softmax(z E^T), every code updated, no counterpart either) the twelfth.

The nearest-codeword search is one exact-fp32 MFMA kernel that never materialises the [N,K] distance
matrix or a one-hot; the reference's association order of the three distance terms is kept so that the
indices are bit-exact.  The EMA statistics are all-reduced over the data-parallel
ranks (a capability the reference lacks -- its ranks silently diverge)."""
import math

import torch
import torch.distributed as dist

from .. import ops
from .abstract_modules.base_quantizer import BaseVectorQuantizer
from .autoencoder import Conv2d


EMA_COLLECTIVES = [0, 0]        # collectives issued / bytes (bench.py reports both per step)


def reduce_ema_stats(stats: torch.Tensor, local_batch: int, force_collective: bool = False) -> float:
    """Collective #2: sum the packed ``[counts(K) | dw(K*D)]`` statistics of every data-parallel rank with
    ONE all-reduce, in place; returns the Laplace-smoothing constant of vector_quantizers.py:164 for the reduced
    statistics = the GLOBAL batch (world * per-rank batch), so that the update equals the reference's single-process EMA
    on the rank-concatenated batch.  Host logic only (no kernel): callable on CPU tensors under gloo."""
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if world > 1 or (force_collective and dist.is_available() and dist.is_initialized()):
        from ..optim import _track
        work = _track(dist.all_reduce(stats, op=dist.ReduceOp.SUM, async_op=True))     # async + wait: see optim.all_reduce_sum
        if work is not None:
            work.wait()
        EMA_COLLECTIVES[0] += 1
        EMA_COLLECTIVES[1] += stats.numel() * stats.element_size()
    return float(local_batch * world)


def gather_latent_sample(rows: torch.Tensor) -> torch.Tensor:
    """The common sample of the data-dependent codebook start (``VQVAE.init_codebook_from_batches``): every data-parallel rank hands
    in the SAME number of latent rows [n, D]; ONE all-gather returns the rank-ordered concatenation [world * n, D] on every rank (the
    rows themselves without a process group).  Host logic only (no kernel): callable on CPU tensors under gloo."""
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if world == 1:
        return rows
    from ..optim import _track
    rows = rows.contiguous()
    out = torch.empty((world * rows.shape[0],) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    work = _track(dist.all_gather(list(out.chunk(world, 0)), rows, async_op=True))      # async + wait: see optim.all_reduce_sum
    if work is not None:
        work.wait()
    return out


def _flat_view(z: torch.Tensor):
    b, d, h, w = z.shape
    return z.permute(0, 2, 3, 1).reshape(b * h * w, d)


GRADIENTS = ('straight_through', 'rotation')


def check_gradient(gradient: str) -> bool:
    """``quantizer.params.gradient`` of the standard and EMA quantizers -> the ``rotate`` flag of ``ops.VQLookupFn``:
    'straight_through' copies the decoder's gradient to the encoder (dz = dq), 'rotation' carries it through the rotation and
    rescaling that maps z onto its code (the rotation trick, Fifty et al., ICLR 2025; csrc/vq_rot.hip).  The forward values, the
    losses, the codebook update and the state dict are the same in both modes."""
    if gradient not in GRADIENTS:
        raise ValueError(f'quantizer.params.gradient must be one of {GRADIENTS}, got {gradient!r}')
    return gradient == 'rotation'


class VectorQuantizer(BaseVectorQuantizer):
    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, gradient: str = 'straight_through'):
        super().__init__(num_embeddings, embedding_dim)
        self.commitment_cost = commitment_cost
        self.gradient, self.rotate = gradient, check_gradient(gradient)

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.VQLookupFn.apply(x, self.codebook.weight, self.commitment_cost, True, 0,
                                                  self.compute_dtype, self.rotate)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return ops.vq_assign(_flat_view(z), self.codebook.weight.detach().contiguous(), 0).view(x.shape[0], -1)


class EMAVectorQuantizer(BaseVectorQuantizer):
    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, decay: float = 0.95,
                 epsilon: float = 1e-5, gradient: str = 'straight_through'):
        super().__init__(num_embeddings, embedding_dim)
        self.commitment_cost = commitment_cost
        self.gradient, self.rotate = gradient, check_gradient(gradient)
        self.codebook.requires_grad_(False)
        self.register_buffer('ema_count', torch.zeros(num_embeddings))
        self.register_buffer('ema_weight', torch.empty(num_embeddings, embedding_dim).uniform_(-1 / num_embeddings,
                                                                                                1 / num_embeddings))
        self.decay = decay
        self.epsilon = epsilon
        # The update only changes what the NEXT step looks up (this step's quantized vectors are already gathered and the
        # backward uses the saved ones), so a trainer may take it out of the forward: with ``defer_update`` the forward
        # leaves this rank's packed statistics in ``pending_stats`` and ``finish_update()`` -- the all-reduce over ranks
        # and the update kernel -- runs after the step's captured graph, next to the gradient all-reduce.
        self.defer_update = False
        self.pending_stats = None
        self._pending_batch = 0

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.VQLookupFn.apply(x, self.codebook.weight, self.commitment_cost, False, 0,
                                                  self.compute_dtype, self.rotate)
        self.last_hist = hist
        if self.training:
            with torch.no_grad():
                z = ops.nhwc(x.detach().to(torch.float32))
                if self.defer_update:
                    self.pending_stats = ops.ema_stats(_flat_view(z), idx.reshape(-1), self.num_embeddings,
                                                       out=self.pending_stats)
                    self._pending_batch = int(x.shape[0])
                else:
                    stats = ops.ema_stats(_flat_view(z), idx.reshape(-1), self.num_embeddings)
                    batch = reduce_ema_stats(stats, int(x.shape[0]))
                    ops.ema_apply(stats, self.ema_count, self.ema_weight, self.codebook.weight.data, self.decay,
                                  self.epsilon, batch)
        return q, idx, loss

    @torch.no_grad()
    def init_codebook_from_data(self, flat_z: torch.Tensor, iters: int, u: torch.Tensor, rows_per_step: int = None) -> dict:
        """the base class's k-means start, plus the running statistics a long run of such batches converges to: ema_count = the
        cluster sizes scaled from the sample to one training step (``rows_per_step`` latent rows over all ranks; default: the sample
        itself), ema_weight = ema_count[:, None] * centres -- so that ema_weight / ema_count reproduces the codebook"""
        fit = super().init_codebook_from_data(flat_z, iters, u, rows_per_step)
        rows = float(flat_z.shape[0] if rows_per_step is None else rows_per_step)
        self.ema_count.copy_(fit['counts'] * (rows / float(flat_z.shape[0])))
        self.ema_weight.copy_(self.ema_count[:, None] * self.codebook.weight.data)
        return fit

    @torch.no_grad()
    def finish_update(self, force_collective: bool = False) -> None:
        """second half of a deferred update: ONE all-reduce of [counts | dw] over the ranks, then the EMA kernel"""
        if self.pending_stats is None:
            return
        batch = reduce_ema_stats(self.pending_stats, self._pending_batch, force_collective)
        ops.ema_apply(self.pending_stats, self.ema_count, self.ema_weight, self.codebook.weight.data, self.decay,
                      self.epsilon, batch)

    vec_to_codes = VectorQuantizer.vec_to_codes           # the same nearest-code assignment


class EntropyVectorQuantizer(BaseVectorQuantizer):
    def __init__(self, num_embeddings: int, embedding_dim: int, ent_loss_ratio: float = 0.1,
                 ent_temperature: float = 0.01, ent_loss_type: str = 'softmax', commitment_cost: float = 0.25):
        super().__init__(num_embeddings, embedding_dim)
        self.ent_loss_ratio = ent_loss_ratio
        self.ent_temperature = ent_temperature
        self.ent_loss_type = ent_loss_type
        self.commitment_cost = commitment_cost

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.EntropyVQFn.apply(x, self.codebook.weight, self.commitment_cost, self.ent_loss_ratio,
                                                   self.ent_temperature, self.compute_dtype, self.ent_loss_type)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return ops.vq_assign(_flat_view(z), self.codebook.weight.detach().contiguous(), 1).view(x.shape[0], -1)


class GumbelVectorQuantizer(BaseVectorQuantizer):
    """Input is the encoder's K-channel logit map (B,K,H,W).  Unlike the other quantizers the indices come back
    shaped (B,H,W) -- the reference's own quirk (vector_quantizers.py:243), kept."""

    def __init__(self, num_embeddings: int, embedding_dim: int, straight_through: bool = False, temp: float = 1.0,
                 kl_cost: float = 5e-4):
        super().__init__(num_embeddings, embedding_dim)
        self.x_to_logits = Conv2d(num_embeddings, num_embeddings, 1, bias=True)
        self.straight_through = straight_through
        self.temp = temp
        self.kl_cost = kl_cost
        self.sched_dev = None          # device [temp, kl_cost]: set by MiniTrainer before a hipGraph capture (replays follow the schedule)

    def enable_device_schedule(self, device) -> torch.Tensor:
        if self.sched_dev is None:
            self.sched_dev = torch.tensor([float(self.temp), float(self.kl_cost)], dtype=torch.float32, device=device)
        return self.sched_dev

    def forward(self, x: torch.Tensor, exp_noise: torch.Tensor = None):
        """``exp_noise`` ~ Exp(1) with the shape of x: injected for parity tests; drawn with torch's RNG otherwise."""
        hard = self.straight_through if self.training else True
        logits = self.x_to_logits(ops.nhwc(x.to(self.compute_dtype)), out_dtype=torch.float32)
        if exp_noise is None:
            exp_noise = torch.empty_like(logits).exponential_()
        q, idx, kl, hist = ops.GumbelVQFn.apply(logits, self.codebook.weight, exp_noise, float(self.temp),
                                                float(self.kl_cost), bool(hard), self.compute_dtype,
                                                self.sched_dev if self.training else None)
        self.last_hist = hist
        return q, idx, kl

    def init_codebook_from_data(self, *args, **kwargs):
        raise ValueError('gumbel: the quantizer does no distance lookup, there is nothing a k-means start of the codebook would serve')

    def get_consts(self):
        return self.temp, self.kl_cost

    def set_consts(self, temp: float = None, kl_cost: float = None) -> None:
        if temp is not None:
            self.temp = temp
        if kl_cost is not None:
            self.kl_cost = kl_cost
        if self.sched_dev is not None:                     # two scalar fills on the stream: no host synchronisation
            self.sched_dev[0:1].fill_(float(self.temp))
            self.sched_dev[1:2].fill_(float(self.kl_cost))

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        """hard Gumbel sample of x itself at tau = 1 (the reference skips x_to_logits here, :272-273)"""
        lg = ops.nhwc(x.to(torch.float32))
        noise = torch.empty_like(lg).exponential_()
        _, idx, _, _ = ops.GumbelVQFn.apply(lg, self.codebook.weight, noise, 1.0, 0.0, True, self.compute_dtype)
        return idx


class _ProjectionQuantizer(BaseVectorQuantizer):
    """What the quantizers without a learned codebook share (``FSQuantizer``, ``LFQuantizer``, ``BSQuantizer``): the D-channel latent is projected to
    ``channels`` channels, every channel is quantized on its own, the token is a number formed from the channels' codes and the code
    vector is projected back to D channels (the kernel core of csrc/proj_quant.h).  The two 1x1 projections are ``Conv2d`` modules for
    their parameters (names, initialisation, weight-decay group) only -- the kernels read their [d, D] / [D, d] weight memory directly.
    ``codebook`` holds the IMPLICIT codebook [K, channels], frozen.  A subclass validates its arguments, then supplies
    ``implicit_codebook()``, ``forward()`` and its assignment / decode operator (``_assign(flat_z)``, ``_decode(codes)``); ``kind``
    words the messages."""
    kind = ''

    def __init__(self, num_embeddings: int, embedding_dim: int, channels: int):
        super().__init__(num_embeddings, channels)            # the codebook the base class owns is the implicit one, frozen
        self.embedding_dim = embedding_dim
        self.codebook.requires_grad_(False)
        self.project_in = Conv2d(embedding_dim, channels, 1, bias=True)      # registration order codebook, project_in, project_out:
        self.project_out = Conv2d(channels, embedding_dim, 1, bias=True)     # the optimizer's arena layout follows it

    @torch.no_grad()
    def init_codebook(self) -> None:
        self.codebook.weight.copy_(self.implicit_codebook())

    def _projections(self):
        return self.project_in.weight, self.project_in.bias, self.project_out.weight, self.project_out.bias

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return self._assign(_flat_view(z)).view(x.shape[0], -1)

    @torch.no_grad()
    def get_codebook(self) -> torch.Tensor:
        """the [K, D] decoder-side vectors: every token decoded"""
        return self.codes_to_vec(torch.arange(self.num_embeddings, dtype=torch.int64, device=self.project_out.weight.device))

    @torch.no_grad()
    def codes_to_vec(self, codes: torch.Tensor) -> torch.Tensor:
        """codes (B,N) -> (B,N,D), by arithmetic on the token (no [K, D] table is built)"""
        return self._decode(codes)

    def reinit_unused_codes(self, codebook_usage: torch.Tensor):
        raise RuntimeError(f'{self.kind}: there is no learned codebook to re-initialise')

    def init_codebook_from_data(self, *args, **kwargs):
        raise ValueError(f'{self.kind}: there is no learned codebook to initialise from data')


class FSQuantizer(_ProjectionQuantizer):
    """Finite scalar quantization (Mentzer et al. 2023): the D-channel latent is projected to ``len(levels)`` channels, each is
    tanh-bounded and rounded to one of its ``levels[j]`` integer values, the mixed-radix number of the rounded vector is the
    token, and the rounded vector is projected back to D channels.  No learned codebook, no latent loss, no dead codes, no
    statistics to all-reduce; training and evaluation behave the same.  One fused kernel each way (csrc/fsq.hip).  ``codebook`` holds
    the IMPLICIT codebook, frozen: row i = the rounded vector of token i, scaled to [-1, 1]."""
    kind = 'fsq'

    def __init__(self, num_embeddings: int, embedding_dim: int, levels):
        levels = [int(v) for v in levels]
        if not 1 <= len(levels) <= 8:
            raise ValueError(f'fsq: between 1 and 8 levels, got {len(levels)}')
        if any(v < 2 for v in levels):
            raise ValueError(f'fsq: every level must be >= 2, got {levels}')
        if math.prod(levels) != num_embeddings:
            raise ValueError(f'fsq: num_embeddings = {num_embeddings} must equal prod(levels) = {math.prod(levels)}')
        super().__init__(num_embeddings, embedding_dim, len(levels))
        self.levels = tuple(levels)
        self.init_codebook()

    def _assign(self, flat_z: torch.Tensor) -> torch.Tensor:
        return ops.fsq_assign(flat_z, self.project_in.weight, self.project_in.bias, self.levels)

    def _decode(self, codes: torch.Tensor) -> torch.Tensor:
        return ops.fsq_decode(codes, self.project_out.weight, self.project_out.bias, self.levels)

    def implicit_codebook(self) -> torch.Tensor:
        """[K, d] fp32: row i = (digit_j(i) - L_j // 2) / (L_j // 2), digit_j the j-th mixed-radix digit of i (first level fastest)"""
        rem = torch.arange(self.num_embeddings, dtype=torch.int64)
        cols = []
        for lv in self.levels:
            cols.append(((rem % lv) - lv // 2).to(torch.float32) / float(lv // 2))
            rem = rem // lv
        return torch.stack(cols, 1)

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.FSQFn.apply(x, *self._projections(), self.levels, self.compute_dtype)
        self.last_hist = hist
        return q, idx, loss


class _SignQuantizer(_ProjectionQuantizer):
    """What the sign quantizers share (``LFQuantizer``, ``BSQuantizer``; kernel core csrc/sign_quant.h): ``bits`` channels quantized
    to their sign, token = the bit pattern, loss = commitment_cost * commit + ent_loss_ratio * (H_sample - diversity_gamma * H_batch).
    A subclass sets ``kind``, its autograd Function ``Fn``, its default ``ent_temperature`` and the scale of the +-1 table in
    ``implicit_codebook()``; ``ops.<kind>_assign`` / ``ops.<kind>_decode`` and ``ops.<KIND>_MAX_*`` are found by ``kind``."""
    Fn = None

    def __init__(self, num_embeddings: int, embedding_dim: int, bits: int, commitment_cost: float, ent_loss_ratio: float,
                 ent_temperature: float, diversity_gamma: float, ent_group_bits: int):
        kind = self.kind
        max_bits, max_group = getattr(ops, f'{kind.upper()}_MAX_BITS'), getattr(ops, f'{kind.upper()}_MAX_GROUP_BITS')
        bits, ent_group_bits = int(bits), int(ent_group_bits)
        if not 1 <= bits <= max_bits:
            raise ValueError(f'{kind}: bits must be between 1 and {max_bits}, got {bits}')
        if num_embeddings != 2 ** bits:
            raise ValueError(f'{kind}: num_embeddings = {num_embeddings} must equal 2**bits = {2 ** bits}')
        if not 1 <= ent_group_bits <= max_group:
            raise ValueError(f'{kind}: ent_group_bits must be between 1 and {max_group}, got {ent_group_bits}')
        if not float(ent_temperature) > 0.0:
            raise ValueError(f'{kind}: ent_temperature must be > 0, got {ent_temperature}')
        super().__init__(num_embeddings, embedding_dim, bits)
        self.bits, self.ent_group_bits = bits, ent_group_bits
        self.commitment_cost, self.ent_loss_ratio = float(commitment_cost), float(ent_loss_ratio)
        self.ent_temperature, self.diversity_gamma = float(ent_temperature), float(diversity_gamma)
        self.last_parts = None
        self.init_codebook()

    def _assign(self, flat_z: torch.Tensor) -> torch.Tensor:
        return getattr(ops, f'{self.kind}_assign')(flat_z, self.project_in.weight, self.project_in.bias, self.bits)

    def _decode(self, codes: torch.Tensor) -> torch.Tensor:
        return getattr(ops, f'{self.kind}_decode')(codes, self.project_out.weight, self.project_out.bias, self.bits)

    def _signs(self) -> torch.Tensor:
        """[K, bits] fp32: row i, column j = +1 if bit j of i is set, else -1"""
        tokens = torch.arange(self.num_embeddings, dtype=torch.int64)
        return (((tokens[:, None] >> torch.arange(self.bits)) & 1) * 2 - 1).to(torch.float32)

    def forward(self, x: torch.Tensor):
        cfg = (self.bits, self.ent_group_bits, self.commitment_cost, self.ent_loss_ratio, self.diversity_gamma, self.ent_temperature)
        q, idx, loss, hist, parts = self.Fn.apply(x, *self._projections(), cfg, self.compute_dtype)
        self.last_hist, self.last_parts = hist, parts
        return q, idx, loss


class LFQuantizer(_SignQuantizer):
    """Lookup-free quantization (Yu et al. 2023, MAGVIT-v2; Open-MAGVIT2): the D-channel latent is projected to ``bits`` channels, each
    is quantized to its sign, the bit pattern is the token (K = 2^bits, first channel = bit 0) and the sign vector is projected back
    to D channels.  loss = commitment_cost * commit + ent_loss_ratio * (H_sample - diversity_gamma * H_batch): the per-position
    entropy keeps the bits confident, the entropy of the batch-average distribution -- factorised over groups of ``ent_group_bits``
    bits -- keeps the vocabulary evenly used.  No learned codebook, no search, no dead codes, no collective (data parallel, the batch
    average is per rank, as the entropy quantizer's statistics are); training and evaluation behave the same.  One fused kernel each
    way (csrc/lfq.hip).  ``codebook`` holds the IMPLICIT codebook, frozen: row i = the +-1 vector of token i.  ``last_parts`` =
    (commit, H_sample, H_batch) of the last forward, on the device, for logging."""
    kind, Fn = 'lfq', ops.LFQFn

    def __init__(self, num_embeddings: int, embedding_dim: int, bits: int, commitment_cost: float = 0.25, ent_loss_ratio: float = 0.1,
                 ent_temperature: float = 0.01, diversity_gamma: float = 1.0, ent_group_bits: int = 9):
        super().__init__(num_embeddings, embedding_dim, bits, commitment_cost, ent_loss_ratio, ent_temperature, diversity_gamma,
                         ent_group_bits)

    def implicit_codebook(self) -> torch.Tensor:
        """[K, bits] fp32: row i, column j = +1 if bit j of i is set, else -1"""
        return self._signs()


class BSQuantizer(_SignQuantizer):
    """Binary spherical quantization (Zhao, Xiong, Kraehenbuehl 2024, BSQ-ViT): ``LFQuantizer`` with the projected latent put on the
    unit sphere before the sign is taken -- u = v / |v|, code = the corner +-1 / sqrt(bits) of the hypercube inscribed in the sphere,
    token = the bit pattern (K = 2^bits, first channel = bit 0).  The quantization error |u - c|^2 is below 2 for every ``bits``, so the
    commitment term (a sum over channels, a mean over positions) keeps its scale as the vocabulary grows; the entropy terms and their
    group factorisation are ``LFQuantizer``'s on the logits 4 u_j / (sqrt(bits) ent_temperature) (``ent_temperature`` 0.02 = the
    paper's inverse temperature 100).  Straight-through at u, the gradient carried through the normalisation.  No learned codebook,
    no search, no collective; training and evaluation behave the same.  One fused kernel each way (csrc/bsq.hip).  ``codebook`` holds
    the IMPLICIT codebook, frozen: row i = the +-1 / sqrt(bits) vector of token i.  ``last_parts`` = (commit, H_sample, H_batch) of the
    last forward, on the device, for logging."""
    kind, Fn = 'bsq', ops.BSQFn

    def __init__(self, num_embeddings: int, embedding_dim: int, bits: int, commitment_cost: float = 0.25, ent_loss_ratio: float = 0.1,
                 ent_temperature: float = 0.02, diversity_gamma: float = 1.0, ent_group_bits: int = 9):
        super().__init__(num_embeddings, embedding_dim, bits, commitment_cost, ent_loss_ratio, ent_temperature, diversity_gamma,
                         ent_group_bits)

    def implicit_codebook(self) -> torch.Tensor:
        """[K, bits] fp32: row i, column j = +1 / sqrt(bits) if bit j of i is set, else -1 / sqrt(bits)"""
        return self._signs() / math.sqrt(self.bits)


class ResidualVectorQuantizer(BaseVectorQuantizer):
    """Residual quantization (Lee et al. 2022, RQ-VAE; SoundStream): every latent vector is approximated by the sum of ``depth`` codes
    of ONE shared codebook, stage q quantizing what the stages before it left over -- K^depth effective codes per position from the
    codebook memory of the standard quantizer, and a coarse-to-fine token stack (B, H*W, depth).  Every stage carries the standard
    quantizer's codebook + commitment loss on its own input residual.  One fused forward kernel for all stages and one backward kernel
    (csrc/rvq.hip).  Depth 1 is the standard quantizer.  The codebook (``codebook.weight``), its initialisation, usage statistics and
    dead-code re-initialisation are the base class's; ``init_codebook_from_data`` is inherited as it is: the shared codebook is fitted
    to z, the FIRST stage's input (the later stages' residuals only exist once there is a codebook): ``last_hist`` is the usage POOLED over the stages (total N * depth),
    ``last_depth_hist`` [depth, K] the per-stage table (later stages collapse first), ``last_stage_sse`` [depth] the residual energy
    sum |r_q|^2 left after each stage."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, depth: int = 4):
        depth = int(depth)
        if not 1 <= depth <= ops.RVQ_MAX_DEPTH:
            raise ValueError(f'residual quantizer: depth must be between 1 and {ops.RVQ_MAX_DEPTH}, got {depth}')
        super().__init__(num_embeddings, embedding_dim)
        self.commitment_cost = commitment_cost
        self.depth = depth
        self.last_depth_hist = None
        self.last_stage_sse = None

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist, depth_hist, stage_sse = ops.RVQLookupFn.apply(x, self.codebook.weight, self.commitment_cost, self.depth,
                                                                          self.compute_dtype)
        self.last_hist, self.last_depth_hist, self.last_stage_sse = hist, depth_hist, stage_sse
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        """x (B,D,H,W) -> codes (B,H*W,depth) int64"""
        z = ops.nhwc(x.to(torch.float32))
        return ops.rvq_assign(_flat_view(z), self.codebook.weight, self.depth).view(x.shape[0], -1, self.depth)

    @torch.no_grad()
    def codes_to_vec(self, codes: torch.Tensor) -> torch.Tensor:
        """codes (B,N,depth) -> (B,N,D): the stage-order sum of the codes, the bits the forward hands to the decoder"""
        if codes.dim() != 3 or not 1 <= codes.shape[-1] <= ops.RVQ_MAX_DEPTH:
            raise ValueError(f'residual quantizer: codes must be (B, N, depth), got {tuple(codes.shape)}')
        return ops.rvq_decode(codes, self.codebook.weight)


class CosineVectorQuantizer(BaseVectorQuantizer):
    """The factorised, l2-normalised codebook of ViT-VQGAN (Yu et al. 2022): the encoder projects to a LOW-dimensional latent
    (``embedding_dim`` 8 to 64 instead of 256), latents and codes are both l2-normalised before the lookup -- the Euclidean ranking is
    then the cosine ranking -- and the decoder sees the normalised code.  loss = codebook term |sg(zn) - en|^2 + ``commitment_cost`` *
    commitment term |zn - sg(en)|^2; the straight-through estimator is taken at the normalised latent.  One fused forward and one
    backward kernel (csrc/vq_cos.hip) for D in {8, 16, 32, 64} and K % 32 == 0, the staged formulation (``ops.cos_staged``) otherwise.
    The state dict is the standard quantizer's: ``codebook.weight`` only, stored UN-normalised, so checkpoints move both ways between
    ``standard`` and ``cosine``.  Usage statistics and dead-code re-initialisation are the base class's.  ``init_codebook_from_data``
    fits k-means to the l2-NORMALISED latent sample (``vqk_l2norm_rows_f32``): Euclidean k-means on the unit sphere, whose centres the
    lookup normalises again (spherical k-means proper is not implemented)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25):
        if int(embedding_dim) % 8 != 0:
            raise ValueError(f'cosine quantizer: embedding_dim must be a multiple of 8, got {embedding_dim}')
        super().__init__(num_embeddings, embedding_dim)
        self.commitment_cost = commitment_cost

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.CosLookupFn.apply(x, self.codebook.weight, self.commitment_cost, self.compute_dtype)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return ops.cos_assign(_flat_view(z), self.codebook.weight).view(x.shape[0], -1)

    @torch.no_grad()
    def codes_to_vec(self, codes: torch.Tensor) -> torch.Tensor:
        """codes (B,N) -> (B,N,D): the NORMALISED code rows, the bits the forward hands to the decoder"""
        return ops.cos_decode(codes, self.codebook.weight)

    @torch.no_grad()
    def init_codebook_from_data(self, flat_z: torch.Tensor, iters: int, u: torch.Tensor, rows_per_step: int = None) -> dict:
        """the base class's k-means start on the l2-normalised sample (see the class docstring)"""
        w = self.codebook.weight
        if flat_z.dim() != 2 or flat_z.shape[1] != w.shape[1]:
            raise ValueError(f'init_codebook_from_data: latents must be [N, {w.shape[1]}], got {tuple(flat_z.shape)}')
        return super().init_codebook_from_data(ops.l2norm_rows(flat_z), iters, u, rows_per_step)


class GroupedVectorQuantizer(BaseVectorQuantizer):
    """Product (multi-codebook, "multi-head") quantization, as in UniTok and wav2vec 2.0: the ``embedding_dim`` = D channels are cut
    into ``groups`` = G contiguous groups of d = D / G channels and each group is looked up in its OWN codebook of ``num_embeddings``
    = K codes; the decoder sees the concatenation and a position carries G tokens -- K^G effective codes from the codebook memory
    (G K d = K D floats) and the lookup FLOP of the standard quantizer.  Every group carries the standard quantizer's codebook +
    commitment loss on its slice; straight-through estimator.  One fused forward and one backward kernel (csrc/gvq.hip) for d in
    {8, 16, 32, 64} and K % 32 == 0, the staged formulation (``ops.gvq_staged``) otherwise.  ``groups = 1`` is the standard quantizer.
    ``codebook.weight`` is [G K, d], row g K + k = code k of group g (at G = 1 the standard quantizer's [K, D] tensor); tokens are
    (B, H*W, G); ``last_hist``, the usage statistics and the dead-code re-initialisation work on the [G K] table, group by group."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, groups: int = 1):
        groups = int(groups)
        if not 1 <= groups <= ops.GVQ_MAX_GROUPS:
            raise ValueError(f'grouped quantizer: groups must be between 1 and {ops.GVQ_MAX_GROUPS}, got {groups}')
        if int(embedding_dim) % groups != 0:
            raise ValueError(f'grouped quantizer: embedding_dim = {embedding_dim} must be a multiple of groups = {groups}')
        super().__init__(groups * int(num_embeddings), int(embedding_dim) // groups)       # the codebook the base class owns: [G K, d]
        self.num_embeddings, self.embedding_dim, self.groups = int(num_embeddings), int(embedding_dim), groups
        self.commitment_cost = commitment_cost

    def init_codebook(self) -> None:
        torch.nn.init.uniform_(self.codebook.weight, -1 / self.num_embeddings, 1 / self.num_embeddings)

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.GVQLookupFn.apply(x, self.codebook.weight, self.commitment_cost, self.groups, self.compute_dtype)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        """x (B,D,H,W) -> codes (B,H*W,G) int64"""
        z = ops.nhwc(x.to(torch.float32))
        return ops.gvq_assign(_flat_view(z), self.codebook.weight, self.groups).view(x.shape[0], -1, self.groups)

    @torch.no_grad()
    def codes_to_vec(self, codes: torch.Tensor) -> torch.Tensor:
        """codes (B,N,G) -> (B,N,D): the concatenated code rows, the bits the forward hands to the decoder"""
        if codes.dim() != 3 or codes.shape[-1] != self.groups:
            raise ValueError(f'grouped quantizer: codes must be (B, N, {self.groups}), got {tuple(codes.shape)}')
        return ops.gvq_decode(codes, self.codebook.weight)

    def tokens_to_hist(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens (..., G) -> the [G K] usage table: entry g K + k counts token k in group g (tokens outside [0, K) count nowhere)"""
        if tokens.shape[-1] != self.groups:
            raise ValueError(f'grouped quantizer: tokens must be (..., {self.groups}), got {tuple(tokens.shape)}')
        k = self.num_embeddings
        t = tokens.reshape(-1, self.groups).to(torch.int64)
        gid = t + torch.arange(self.groups, device=t.device, dtype=torch.int64) * k
        return torch.bincount(gid[(t >= 0) & (t < k)], minlength=self.groups * k)

    def get_codebook_usage(self, index_count: torch.Tensor):
        """index_count (G K,) -> (usage probabilities (G K,), normalised PER GROUP; the mean of the per-group perplexities; the
        percentage of all G K rows in use)"""
        cnt = index_count.reshape(self.groups, self.num_embeddings)
        p = cnt / torch.sum(cnt, dim=1, keepdim=True)
        perplexity = torch.exp(-torch.sum(p * torch.log(p + 1e-10), dim=1)).mean().item()
        used = torch.count_nonzero(p).item() * 100 / index_count.shape[0]
        return p.reshape(-1), perplexity, used

    @torch.no_grad()
    def reinit_unused_codes(self, codebook_usage: torch.Tensor):
        """a dead code is overwritten with a code of ITS OWN group, sampled in proportion to that group's usage (a group without a
        single live code is left alone).  Data parallel: the draw is made on rank 0 and broadcast, as in the base class."""
        k = self.num_embeddings
        usage = codebook_usage.reshape(self.groups, k)
        dead, picks = [], []
        for g in range(self.groups):
            unused = torch.nonzero(usage[g] == 0).squeeze(1)
            if unused.numel() == 0 or unused.numel() == k:
                continue
            dead.append(unused + g * k)
            picks.append(torch.multinomial(usage[g].float(), unused.numel(), replacement=True) + g * k)
        if not dead:
            return
        dead, picks = torch.cat(dead), torch.cat(picks)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from ..optim import broadcast_
            broadcast_(picks, src=0)                 # async + wait: no event on a stream that may capture next (optim.all_reduce_sum)
        self.codebook.weight[dead] = self.codebook.weight[picks]

    @torch.no_grad()
    def init_codebook_from_data(self, flat_z: torch.Tensor, iters: int, u: torch.Tensor, rows_per_step: int = None) -> dict:
        """Data-dependent start, group by group: slab g becomes the k-means centres of the contiguous slice flat_z[:, g d:(g + 1) d]
        (``ops.kmeans_fit`` with the draws u[g K:(g + 1) K]; ``u`` holds G K float64 draws).  Written in place and broadcast from rank
        0 as in the base class.  Returns dict(centres [G K, d], counts [G K], inertia = the groups' sum, used = the used fraction of
        all G K centres)."""
        w = self.codebook.weight
        k, d = self.num_embeddings, w.shape[1]
        if flat_z.dim() != 2 or flat_z.shape[1] != self.embedding_dim:
            raise ValueError(f'init_codebook_from_data: latents must be [N, {self.embedding_dim}], got {tuple(flat_z.shape)}')
        if u.numel() != self.groups * k:
            raise ValueError(f'init_codebook_from_data: {self.groups * k} draws are needed ({self.groups} groups of {k}), got {u.numel()}')
        z = flat_z.detach().to(torch.float32)
        fits = [ops.kmeans_fit(z[:, g * d:(g + 1) * d].contiguous(), k, iters, u[g * k:(g + 1) * k]) for g in range(self.groups)]
        fit = dict(centres=torch.cat([f['centres'] for f in fits]), counts=torch.cat([f['counts'] for f in fits]).to(torch.float32),
                   inertia=sum(f['inertia'] for f in fits), used=sum(f['used'] for f in fits) / self.groups)
        w.data.copy_(fit['centres'])
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from ..optim import broadcast_
            broadcast_(w.data, src=0)
            broadcast_(fit['counts'], src=0)
        return fit


class SimVectorQuantizer(BaseVectorQuantizer):
    """SimVQ (Zhu et al. 2024, "Addressing representation collapse in vector quantized models with one linear layer"): the code table
    ``codebook.weight`` = C [K, D] is FROZEN at its random start and one linear layer ``codebook_proj`` (W [D, D], optional bias b) is
    learned; the effective codebook is E = C W^T + b, so every optimizer step moves EVERY code and neither dead-code
    re-initialisation nor a data-dependent start is needed (both raise).  The lookup against E, the codebook + commitment loss and the
    straight-through estimator are the standard quantizer's; the backward is the gather-GEMM pair of csrc/simvq.hip for D in
    {64, 128, 256} and K % 32 == 0 (the torch closed forms otherwise), E comes from torch.addmm unless ``ops.SIMVQ_PROJECT`` asks for
    the HIP projection (the measured keep decision).  Tokens are (B, H*W)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, proj_bias: bool = True):
        super().__init__(int(num_embeddings), int(embedding_dim))
        self.commitment_cost = commitment_cost
        self.codebook.requires_grad_(False)                    # the frozen table: same state-dict key as every other quantizer
        self.codebook_proj = torch.nn.Linear(self.embedding_dim, self.embedding_dim, bias=bool(proj_bias))

    @torch.no_grad()
    def init_codebook(self) -> None:
        """C ~ N(0, 1 / D); W = I, b = 0: at step 0 a standard quantizer over a Gaussian table (this module's own choice)"""
        torch.nn.init.normal_(self.codebook.weight, 0.0, self.embedding_dim ** -0.5)
        torch.nn.init.eye_(self.codebook_proj.weight)
        if self.codebook_proj.bias is not None:
            torch.nn.init.zeros_(self.codebook_proj.bias)

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.SimVQLookupFn.apply(x, self.codebook.weight, self.codebook_proj.weight, self.codebook_proj.bias,
                                                     self.commitment_cost, self.compute_dtype)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def get_codebook(self) -> torch.Tensor:
        """the EFFECTIVE codebook E [K, D] of the current parameters (a fresh tensor; the forward's bits)"""
        return ops.simvq_effective(self.codebook.weight, self.codebook_proj.weight, self.codebook_proj.bias)

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return ops.simvq_assign(_flat_view(z), self.codebook.weight, self.codebook_proj.weight, self.codebook_proj.bias).view(x.shape[0], -1)

    def reinit_unused_codes(self, codebook_usage: torch.Tensor):
        raise RuntimeError('simvq: the code table is frozen -- there is no dead-code re-initialisation (reinit_every_n_epochs must be empty)')

    def init_codebook_from_data(self, flat_z: torch.Tensor, iters: int, u: torch.Tensor, rows_per_step: int = None) -> dict:
        raise RuntimeError('simvq: the code table is frozen at its random start -- there is no data-dependent codebook_init')


class IBQuantizer(BaseVectorQuantizer):
    """Index backpropagation (IBQ): the token is the argmax of softmax(z E^T / T) over the learned codebook ``codebook.weight`` =
    E [K, D], the output the gathered code, and the one-hot is made differentiable with a straight-through estimator on the softmax --
    so every optimizer step moves EVERY code and the encoder is trained through the logits, not through a copy of the decoder's
    gradient.  loss = (2 + beta) / (N D) sum |q - z|^2.  The lookup ranks dot products, not distances.  Fused HIP kernels that never
    hold an N x K array for D in {64, 128, 256} (csrc/ibq.hip), the staged torch formulation otherwise.  Tokens are
    (B, H*W); the uniform start, usage statistics, dead-code re-initialisation and ``codes_to_vec`` are the base class's."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, temperature: float = 1.0):
        super().__init__(int(num_embeddings), int(embedding_dim))
        self.commitment_cost = float(commitment_cost)
        self.temperature = float(temperature)
        if not (self.temperature > 0.0 and self.temperature < math.inf):
            raise ValueError(f'ibq: temperature must be a positive finite number, got {temperature!r}')

    def forward(self, x: torch.Tensor):
        q, idx, loss, hist = ops.IBQLookupFn.apply(x, self.codebook.weight, self.commitment_cost, self.temperature, self.compute_dtype)
        self.last_hist = hist
        return q, idx, loss

    @torch.no_grad()
    def vec_to_codes(self, x: torch.Tensor) -> torch.Tensor:
        z = ops.nhwc(x.to(torch.float32))
        return ops.ibq_assign(_flat_view(z), self.codebook.weight, self.temperature).view(x.shape[0], -1)

    def init_codebook_from_data(self, flat_z: torch.Tensor, iters: int, u: torch.Tensor, rows_per_step: int = None) -> dict:
        raise RuntimeError('ibq: the lookup ranks dot products, not distances -- there is no k-means codebook_init')
