"""Policy-gradient fine-tuning on what the sampler drew: the per-molecule objective the ELBO trainer (trainer1.py) does
not have.  `reinforce_loss` is the REINFORCE surrogate over differentiable sequence log-likelihoods
(decode.sequence_logp -> gct_seq_logp_bwd), `reinforce_step` one update of a sampler's model on rows it decoded:

    out = sampler.sample_smiles(..., return_rows=True)          # ..., DecodedRows
    reward = torch.tensor([score(s) for s in out[0]])           # any per-molecule number
    stats = reinforce_step(sampler, optimizer, out[-1], reward)

A reward alone collapses the policy onto the few strings that earn it.  The two standard remedies need the whole
next-token distribution at every scored token, not logp: an entropy bonus on the policy and a KL penalty that ties it to
a frozen copy of the pretrained model (decode.sequence_policy -> gct_seq_dist / gct_seq_dist_bwd, from the one forward
logp takes):

    prior = frozen_prior(sampler.model)                         # before the first update
    stats = reinforce_step(sampler, optimizer, out[-1], reward, entropy_coef=0.05, kl_coef=0.5, prior=prior)

`regularised_loss` is the loss of that step; REINVENT-style augmented likelihoods are functions of
`sampler.policy_terms(*rows, prior=prior)`'s logp and prior_logp.  Reward-weighted likelihood, hill-climbing on the best
k of a batch and any other per-molecule loss are functions of `sampler.logp(*rows).logp` in the same way.

One update per scored batch throws the batch away while the reward is the expensive part.  `ppo_update` takes several
updates on it -- PPO's clipped surrogate holds each token's probability ratio against the sampling-time policy inside a
trust region (decode.sequence_ppo -> gct_seq_ppo / gct_seq_ppo_bwd; `advantages` and `ppo_loss` are its pieces):

    history = ppo_update(sampler, optimizer, out[-1], reward, epochs=4, clip=0.2)

Both take max_grad_norm, the bound on the global L2 norm of an update's gradient that PPO and REINFORCE recipes carry:
a FusedAdam clips on the device (optim.py: no host read, a non-finite norm skips the update), any other optimizer gets
torch.nn.utils.clip_grad_norm_.

A sharpened policy fills a sampled batch with copies of a few strings.  `sampler.decode_unique(..., return_rows=True)`
draws k DISTINCT molecules per latent instead (stochastic beam search), and decode.sbs_importance_weights turns them into
an unbiased estimate of the ordinary objective -- a loss weighted that way, every row scored once:

    sbs, rows = sampler.decode_unique(zs, ys0, src_mask, dconds, k=16, return_rows=True)
    w, _ = sbs_importance_weights(sbs.logp, sbs.gumbel)         # [n, k]; reward [n * k], sample-major like the rows
    loss = -(w.view(-1) * (reward - reward.mean()) * sampler.logp(*rows).logp).sum() / w.shape[0]

Rows drawn through top-k / nucleus / temperature or the grammar come from a behaviour distribution q that is not the
policy pi, so a policy gradient on them is biased.  A sampler built with with_logp=True, with_stats=True reports both
log-probabilities of every row, and `behaviour_weights` turns them into the importance weights rho = pi(x) / q(x) that
both update functions take per molecule:

    smiles, _, _, logp, stats, rows = sampler.sample_smiles(..., return_rows=True)
    rho = behaviour_weights(logp, stats.behaviour_logp_sum, clip=5.0)
    stats = reinforce_step(sampler, optimizer, rows, reward, weight=rho)

Not covered: FlatDataParallel fine-tuning, value networks / GAE (the advantage is per molecule),
sequence-level ratios (functions of logp and the old logp in torch), rows of deterministic beam search, a gradient into
the prior or into old_token_logp."""
import copy

import torch

from .. import ops
from ..decode import clip_pair
from ..molkey import first_occurrence
from ..optim import FusedAdam, check_max_grad_norm


class _GradClip:
    """max_grad_norm of reinforce_step / ppo_update.  A FusedAdam clips on the device (its max_grad_norm is set for the
    duration of the call and put back by restore(); a call that passes None leaves the optimizer's own setting in
    force); any other optimizer gets torch.nn.utils.clip_grad_norm_ over its parameters between backward() and step().
    active: whether anything clips.  After a step(), norm_and_clipped() is two device scalars for the caller's one
    transfer: the pre-clip norm and 1.0 where the update was scaled down (0 < coef < 1; a step skipped for a norm that
    is not finite reports that norm and 0)."""

    def __init__(self, optimizer, max_grad_norm, what):
        value = check_max_grad_norm(max_grad_norm, f"{what}: max_grad_norm")
        self.optimizer, self.fused = optimizer, isinstance(optimizer, FusedAdam)
        self.saved = optimizer.max_grad_norm if self.fused else None
        self.value = value if value is not None else check_max_grad_norm(self.saved, f"{what}: optimizer.max_grad_norm")
        self.active = self.value is not None
        self._norm = None

    def install(self):
        if self.fused:
            self.optimizer.max_grad_norm = self.value

    def restore(self):
        if self.fused:
            self.optimizer.max_grad_norm = self.saved

    def step(self):
        if self.active and not self.fused:
            params = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
            self._norm = (torch.nn.utils.clip_grad_norm_(params, self.value).detach().float() if params
                          else torch.zeros(()))                 # no gradient anywhere: norm 0, nothing clipped
        self.optimizer.step()

    def norm_and_clipped(self):
        if self.fused and self.optimizer.clip_state is None:    # a generic-path FusedAdam without any gradient
            return torch.zeros(()), torch.zeros(())
        if self.fused:
            norm, coef = self.optimizer.clip_state[0], self.optimizer.clip_state[1]
        else:
            norm = self._norm
            coef = torch.where(torch.isfinite(norm), (self.value / (norm + 1e-6)).clamp(max=1.0), torch.zeros_like(norm))
        return norm.clone(), ((coef > 0) & (coef < 1)).float()


def behaviour_weights(model_logp, behaviour_logp, clip=None):
    """Per-molecule importance weights rho [n] = exp(model_logp - behaviour_logp) of rows sampled from a behaviour
    distribution that is not the policy (a top-k / nucleus / temperature filter, the grammar): model_logp [n] the
    policy's log-probability of each row (with_logp), behaviour_logp [n] the one under the distribution it was drawn
    from (StepStats.behaviour_logp_sum).  clip (a finite number > 0, optional): rho is truncated at that value --
    truncated importance sampling, a bounded variance for a bias towards the behaviour policy.  fp32, no graph, on the
    device of model_logp.  ValueError for shapes that do not match, values that are not finite and a bad clip."""
    lp = torch.as_tensor(model_logp).detach().float()
    lq = torch.as_tensor(behaviour_logp).detach().float().to(lp.device)
    if lp.dim() != 1 or lp.shape != lq.shape:
        raise ValueError(f"behaviour_weights: model_logp {list(lp.shape)} and behaviour_logp {list(lq.shape)} must be "
                         "vectors of one length")
    if not (bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lq).all())):
        raise ValueError("behaviour_weights: the log-probabilities must be finite")
    if clip is not None:
        if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not 0.0 < float(clip) < float("inf"):
            raise ValueError(f"behaviour_weights: clip must be a finite number > 0 or None, got {clip!r}")
    rho = torch.exp(lp - lq)
    return rho if clip is None else rho.clamp(max=float(clip))


def validity_reward(report, shaped=False, lengths=None):
    """One reward per row from a smiles.ChemReport (Sampling.check_rows): fp32 [n] on the report's device, no graph and
    no synchronisation -- reinforce_step / ppo_update take it as `reward` as it is.  1 where status == ops.CHEM_OK, else
    0.  shaped=True: a rejected row gets position / length instead, the share of its span that lies in front of the
    first offence; lengths ints [n] (or one int) are the span lengths W - prefix_lens, all >= 1.  (A SYNTAX row that
    never reached <eos> has position == length: rows decoded with well_formed=True have none.)  ValueError for
    shaped=True without lengths, or lengths of another shape."""
    status = report.status
    ok = status == ops.CHEM_OK
    if not shaped:
        return ok.float()
    if lengths is None:
        raise ValueError("validity_reward: shaped=True needs the span lengths")
    lengths = torch.as_tensor(lengths)
    if lengths.dtype.is_floating_point or lengths.numel() not in (1, status.numel()) or (
            not lengths.is_cuda and lengths.numel() and int(lengths.min()) < 1):
        raise ValueError(f"validity_reward: lengths must be ints >= 1, one or one per row ({status.numel()}), got "
                         f"{lengths.dtype} {list(lengths.shape)}")
    share = report.position.float() / lengths.reshape(-1).to(status.device, non_blocking=True).float()
    return torch.where(ok, torch.ones_like(share), share)


def uniqueness_reward(keys, index=None, group=None):
    """One reward per row from molecule keys (Sampling.molecule_keys: a MolKeys, or int64 [n]): fp32 [n] on the keys'
    device, no graph and no synchronisation -- to multiply into validity_reward.  1 on the first row of the batch that
    holds a key (per `group`, ints [n], when given: per scaffold or per condition), and with index (a molkey.MolKeyIndex
    of the training set) only if the index does not hold the key; else 0.  A policy that writes one molecule in five
    spellings is paid once."""
    first = first_occurrence(keys, group)
    if index is not None:
        first = first & ~index.contains(keys)
    return first.float()


def scaffold_reward(sca):
    """One reward per row from a scaffold.ScaffoldRows of `scaffold <sep> molecule` rows (Sampling.scaffold_report): fp32
    [n] on the rows' device, no graph and no synchronisation -- to multiply into validity_reward.  1 where the molecule
    has the scaffold it was given (scaffold.scaffold_match: a scaffold was extracted, the given part has a graph, and
    the two keys are equal), else 0: a row without a given scaffold is never paid."""
    from ..scaffold import scaffold_match
    return scaffold_match(sca).float()


def similarity_reward(agg_or_best, lo=0.0, hi=1.0):
    """One reward per row from its largest Tanimoto similarity to a target set (a fingerprint.TanimotoAgg of
    tanimoto_agg(rows, targets), or its `best`, or FingerprintIndex.nearest's): fp32 [n] on the rows' device, no graph
    and no synchronisation -- to multiply into validity_reward.  `best` clamped to [lo, hi] and rescaled to [0, 1]: 0 up
    to lo, 1 from hi on, linear between.  A row without a fingerprint has best 0.  ValueError unless 0 <= lo < hi <= 1."""
    lo, hi = float(lo), float(hi)
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError(f"similarity_reward: 0 <= lo < hi <= 1, got lo = {lo}, hi = {hi}")
    best = agg_or_best.best if hasattr(agg_or_best, "best") else torch.as_tensor(agg_or_best)
    if best.dim() != 1 or not best.dtype.is_floating_point:
        raise ValueError(f"similarity_reward: best must be a floating-point vector [n], got {best.dtype} {list(best.shape)}")
    return ((best.detach().float().clamp(lo, hi) - lo) / (hi - lo))


def property_reward(desc, name, target, tol):
    """One reward per row from a descriptor.DescRows (Sampling.descriptors): fp32 [n] on the rows' device, no graph and
    no synchronisation -- to multiply into validity_reward.  max(0, 1 - |value - target| / tol) of column `name` (as
    DescRows.column takes it: `tpsa`, `mw`, `hbd`, ...), computed in fp64 (whose division is correctly rounded on every
    device: a GPU's reward and the host's agree to the bit) and rounded once to fp32; 0 where the row is not DESC_OK.
    target: a number, or a tensor with one entry per row, so that a batch of mixed targets works.  ValueError unless
    tol > 0."""
    tol = float(tol)
    if not tol > 0.0:
        raise ValueError(f"property_reward: tol must be positive, got {tol}")
    value = desc.column(name, torch.float64).detach()
    target = torch.as_tensor(target).to(value.device).to(torch.float64)
    if target.dim() > 1 or (target.dim() == 1 and target.numel() != value.numel()):
        raise ValueError(f"property_reward: target must be a number or one per row ({value.numel()}), got "
                         f"{list(target.shape)}")
    reward = (1.0 - (value - target).abs() / tol).clamp(min=0.0).to(torch.float32)
    return torch.where(desc.ok, reward, torch.zeros_like(reward))


def _check_weight(weight, n, what):
    """weight [n] of reinforce_step / ppo_update as an fp32 vector without a graph; ValueError for another length or a
    value that is negative or not finite."""
    w = torch.as_tensor(weight).detach().float().reshape(-1)
    if w.numel() != n:
        raise ValueError(f"{what}: {w.numel()} weights for {n} sequences")
    if not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError(f"{what}: the weights must be finite and >= 0")
    return w


def reinforce_loss(logp, reward, baseline="mean", weight=None):
    """-((reward - b) * logp).sum() / n over the n sequences of a batch: minimising it raises the log-likelihood of the
    sequences whose reward lies above the baseline b and lowers that of the others.  logp [n] (with a graph), reward [n]
    numbers (no gradient flows into them); baseline "mean": the batch mean of the reward, a float or a tensor
    (broadcast against reward): that value, None: 0.  weight [n] (optional, behaviour_weights): each sequence's
    advantage reward - b is multiplied by its weight, after the baseline; None: the unweighted loss, bit for bit."""
    reward = torch.as_tensor(reward, dtype=logp.dtype).to(logp.device).detach().view(-1)
    if reward.numel() != logp.numel():
        raise ValueError(f"{reward.numel()} rewards for {logp.numel()} sequences")
    if baseline is None:
        b = 0.0
    elif isinstance(baseline, str):
        if baseline != "mean":
            raise ValueError(f"baseline must be 'mean', a number, a tensor or None, got {baseline!r}")
        b = reward.mean()
    else:
        b = torch.as_tensor(baseline, dtype=logp.dtype).to(logp.device).detach()
    if weight is None:
        return -((reward - b) * logp.view(-1)).sum() / logp.numel()
    weight = _check_weight(weight, logp.numel(), "reinforce_loss").to(logp.device, logp.dtype)
    return -((weight * (reward - b)) * logp.view(-1)).sum() / logp.numel()


def frozen_prior(model):
    """A frozen copy of `model` to regularise against (sequence_policy's `prior`): in eval() mode, every parameter with
    requires_grad=False, sharing no storage with `model` (copy.deepcopy, which FlatModelMixin keeps sound: a flat
    buffer, planes and hooks of its own), its state_dict equal to model's at the time of the call."""
    prior = copy.deepcopy(model)
    prior.eval()
    for p in prior.parameters():
        p.requires_grad_(False)
    return prior


def regularised_loss(terms, reward, baseline="mean", entropy_coef=0.0, kl_coef=0.0, weight=None):
    """reinforce_loss(terms.logp, reward, baseline, weight) + (kl_coef * terms.kl.sum() - entropy_coef * terms.entropy.sum()) / n
    over the n sequences of a PolicyTerms (decode.sequence_policy): the REINFORCE surrogate, minus an entropy bonus on
    the policy's next-token distributions, plus a penalty on their KL divergence from the prior's -- both summed over
    the scored tokens.  A coefficient of 0 leaves its term out (terms.kl may then be None); kl_coef != 0 needs terms
    computed with a prior, entropy_coef != 0 terms with the entropy: ValueError otherwise."""
    loss = reinforce_loss(terms.logp, reward, baseline, weight)
    n = terms.logp.numel()
    if kl_coef != 0:
        if terms.kl is None:
            raise ValueError("regularised_loss: kl_coef needs terms computed with a prior")
        loss = loss + kl_coef * terms.kl.sum() / n
    if entropy_coef != 0:
        if terms.entropy is None:
            raise ValueError("regularised_loss: entropy_coef needs terms computed with the entropy")
        loss = loss - entropy_coef * terms.entropy.sum() / n
    return loss


def reinforce_step(sampler, optimizer, rows, reward, baseline="mean", entropy_coef=0.0, kl_coef=0.0, prior=None,
                   max_grad_norm=None, weight=None):
    """One policy-gradient update of sampler.model on the decoded rows `rows` (a DecodedRows, or any argument tuple of
    Sampling.logp) with one reward per row: model.train(), sampler.logp(*rows), optimizer.zero_grad(set_to_none=True),
    reinforce_loss -> backward -> optimizer.step(), model.eval().  Returns dict(loss, mean_reward, mean_logp, tokens),
    Python numbers read in ONE transfer (tokens: the scored tokens of the batch).

    entropy_coef / kl_coef / prior (a frozen_prior of the pretrained model): with a coefficient that is not 0, or a
    prior, the step takes sampler.policy_terms(*rows, prior=prior) instead -- the same one forward of the model, one
    more forward-only pass of the prior -- and minimises regularised_loss.  The result then also holds mean_entropy
    and, with a prior, mean_kl (both per scored token: the batch sum / tokens) and mean_prior_logp (per sequence), read
    in the same one transfer.  kl_coef != 0 without a prior: ValueError before any device work.  With the defaults the
    step is the unregularised one, bit for bit.

    max_grad_norm: a bound on the global L2 norm of the update's gradient (clip_grad_norm_'s rule).  A FusedAdam clips
    on the device -- the value is set on the optimizer for this call and put back afterwards, an exception included;
    None leaves an optimizer's own max_grad_norm in force -- and skips the update when the norm is not finite; any
    other optimizer gets torch.nn.utils.clip_grad_norm_ over its parameters between backward() and step().  Whenever
    clipping is active the result also holds grad_norm (pre-clip) and clipped (bool: the update was scaled down), read
    in the same one transfer.  Not a finite number > 0: ValueError before any device work.

    weight [n] (optional; behaviour_weights of rows drawn through a filter or the grammar): every molecule's advantage
    is multiplied by its weight after the baseline (reinforce_loss).  The result then also holds weight_mean and
    weight_max, read in the same one transfer.  None: the step as it is without, bit for bit.  A wrong length or a
    value that is negative or not finite: ValueError before any device work.

    The model runs in training mode, so its dropout is live in this forward: the logp of the step is not the eval-mode
    number `with_logp` reported for the same rows (build the model with dropout 0 where the two must agree).  The prior
    stays in the mode it is in: eval().  ppo_update, whose objective is a ratio against a deterministic old policy,
    runs the model in eval() instead (its train_mode flag).

    What keeps the encoder still: the rows' latents are inputs, so the graph holds the decoder and model.out only and
    the encoder's parameters get NO gradient.  A FRESH optimizer therefore leaves them bit-unchanged (FusedAdam and
    torch's Adam: a zero gradient on zero moments is a zero update).  An optimizer with LOADED moments does not: Adam
    goes on moving a parameter along its first moment when the gradient is zero -- give such a run an optimizer over
    the decoder's and model.out's parameters only, or start it fresh.

    Sampling after an update: the next sample_smiles uses the new weights -- KVDecoder's folded cross-attention
    projections are keyed on model.weights_token(), which follows FusedAdam's kernel and torch's in-place optimizers.
    It does NOT follow writes through `p.data` (KVDecoder.start): whoever updates the weights that way calls
    model.invalidate_weight_planes() before the next decode."""
    model = sampler.model
    if kl_coef != 0 and prior is None:
        raise ValueError("reinforce_step: kl_coef needs a prior (frozen_prior of the pretrained model)")
    gclip = _GradClip(optimizer, max_grad_norm, "reinforce_step")
    reward = torch.as_tensor(reward, dtype=torch.float32)
    if weight is not None:
        weight = _check_weight(weight, reward.numel(), "reinforce_step")
    plain = entropy_coef == 0 and kl_coef == 0 and prior is None
    model.train()
    gclip.install()
    try:
        scores = sampler.logp(*rows) if plain else sampler.policy_terms(*rows, prior=prior)
        optimizer.zero_grad(set_to_none=True)
        loss = (reinforce_loss(scores.logp, reward, baseline, weight) if plain else
                regularised_loss(scores, reward, baseline, entropy_coef, kl_coef, weight))
        loss.backward()
        gclip.step()
    finally:
        gclip.restore()
        model.eval()
    dev = scores.logp.device
    tokens = scores.tokens.sum().float()
    stats = [loss.detach().float(), reward.to(dev).mean(), scores.logp.detach().mean(), tokens]
    if not plain:
        stats.append(scores.entropy.detach().sum() / tokens)
        if prior is not None:
            stats += [scores.kl.detach().sum() / tokens, scores.prior_logp.mean()]
    if gclip.active:
        stats += [t.to(dev) for t in gclip.norm_and_clipped()]
    if weight is not None:                                  # (at the end: the indices in front of them stay)
        stats += [weight.to(dev).mean(), weight.to(dev).max()]
        *stats, w_mean, w_max = torch.stack(stats).cpu().tolist()
    else:
        stats = torch.stack(stats).cpu().tolist()
    out = dict(loss=stats[0], mean_reward=stats[1], mean_logp=stats[2], tokens=int(stats[3]))
    if not plain:
        out["mean_entropy"] = stats[4]
        if prior is not None:
            out["mean_kl"], out["mean_prior_logp"] = stats[5], stats[6]
    if gclip.active:
        out["grad_norm"], out["clipped"] = stats[-2], bool(stats[-1])
    if weight is not None:
        out["weight_mean"], out["weight_max"] = w_mean, w_max
    return out


def advantages(reward, baseline="mean", normalize=False):
    """One advantage per sequence: reward - b with reinforce_loss's baseline rule ("mean": the batch mean of the reward,
    a float or a tensor broadcast against reward: that value, None: 0), fp32 [n] on the device of reward, no graph.
    normalize=True divides by (the batch standard deviation of the advantage, the population one, + 1e-8)."""
    reward = torch.as_tensor(reward, dtype=torch.float32).detach().view(-1)
    if baseline is None:
        adv = reward.clone()
    elif isinstance(baseline, str):
        if baseline != "mean":
            raise ValueError(f"baseline must be 'mean', a number, a tensor or None, got {baseline!r}")
        adv = reward - reward.mean()
    else:
        b = torch.as_tensor(baseline, dtype=torch.float32).to(reward.device).detach()
        if b.numel() not in (1, reward.numel()):
            raise ValueError(f"baseline of shape {list(b.shape)} against {reward.numel()} rewards")
        adv = reward - b.reshape(-1)
    if normalize:
        adv = adv / (adv.std(unbiased=False) + 1e-8)
    return adv


def ppo_loss(terms, entropy_coef=0.0, kl_coef=0.0):
    """(-terms.surrogate.sum() + kl_coef * terms.kl.sum() - entropy_coef * terms.entropy.sum()) / n over the n sequences
    of a PpoTerms (decode.sequence_ppo): minus PPO's clipped surrogate, plus regularised_loss's penalty and bonus.  A
    coefficient of 0 leaves its term out (terms.kl / terms.entropy may then be None); kl_coef != 0 needs terms computed
    with a prior, entropy_coef != 0 terms with the entropy: ValueError otherwise."""
    total = -terms.surrogate.sum()
    if kl_coef != 0:
        if terms.kl is None:
            raise ValueError("ppo_loss: kl_coef needs terms computed with a prior")
        total = total + kl_coef * terms.kl.sum()
    if entropy_coef != 0:
        if terms.entropy is None:
            raise ValueError("ppo_loss: entropy_coef needs terms computed with the entropy")
        total = total - entropy_coef * terms.entropy.sum()
    return total / terms.surrogate.numel()


def _row_slice(rows, lo, hi):
    """Rows lo .. hi - 1 of every per-row element of an argument tuple of Sampling.logp (None stays None)."""
    return tuple(None if a is None else a[lo:hi] for a in rows)


def ppo_update(sampler, optimizer, rows, reward, epochs=4, clip=0.2, baseline="mean", normalize=False,
               old_token_logp=None, minibatch=None, target_kl=None, entropy_coef=0.0, kl_coef=0.0, prior=None,
               train_mode=False, max_grad_norm=None, weight=None):
    """Several policy updates of sampler.model on ONE scored batch: `epochs` passes over the decoded rows `rows` (a
    DecodedRows, or any argument tuple of Sampling.logp) with one reward per row, each pass minimising ppo_loss --
    PPO's clipped surrogate of every scored token's probability ratio against the sampling-time policy, which holds the
    later passes inside a trust region around the policy that drew the rows.  The expensive parts of a round, the decode
    and the reward, are paid once.

    advantage = advantages(reward, baseline, normalize), once.  old_token_logp [n, W]: the log-probabilities the rows
    were sampled with; None takes them from ONE sampler.logp forward under no_grad before the first update, in the mode
    the updates run in -- the first update's ratios are then exactly 1 and its step is reinforce_step's.  A caller may
    pass a table of its own, `sampler.score(*rows).token_logp` for example.  clip: a number e (ratios are held in
    [1 - e, 1 + e]) or a pair (clip_lo, clip_hi).  minibatch=m splits the rows, in order, into ceil(n / m) updates per
    epoch, each normalised by its own row count.  target_kl: no further epoch is started once an epoch's approx_kl (as
    reported below) exceeded it.  entropy_coef / kl_coef / prior as in reinforce_step; kl_coef != 0 without a prior:
    ValueError before any device work.

    The model runs in eval() unless train_mode=True: with live dropout the ratio against a deterministic old policy is
    noise around 1 that the clip then cuts at random -- nobody wants that; reinforce_step, which has no ratio, trains in
    train() (its note on dropout).  train_mode=True is for dropout-0 models and for reproducing reinforce_step.  The
    model is always left in eval().  reinforce_step's notes on the encoder (no gradient: the latents are inputs), on
    optimizers with loaded moments and on sampling after an update hold here unchanged.

    Returns a list with one dict per epoch run, Python numbers read in ONE transfer per epoch: loss (the row-weighted
    mean of the minibatches' losses), mean_surrogate (per sequence), clip_fraction (clipped tokens / scored tokens),
    approx_kl (the k3 estimate of KL(old || new) per scored token, each minibatch measured at its own forward), tokens;
    with entropy_coef != 0 mean_entropy, with a prior mean_kl (both per scored token) and mean_prior_logp (per
    sequence).

    max_grad_norm as in reinforce_step, applied to every minibatch update; whenever clipping is active each epoch's
    dict also holds grad_norm (the largest pre-clip norm over the epoch's minibatch updates) and clipped_updates (how
    many of them were scaled down), read in the same one transfer.

    weight [n] (optional; behaviour_weights): every molecule's advantage is multiplied by its weight, once, after the
    baseline and the normalisation; each epoch's dict then also holds weight_mean and weight_max.  None: the update as
    it is without, bit for bit."""
    model = sampler.model
    if kl_coef != 0 and prior is None:
        raise ValueError("ppo_update: kl_coef needs a prior (frozen_prior of the pretrained model)")
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"epochs must be an int >= 1, got {epochs!r}")
    if minibatch is not None and (isinstance(minibatch, bool) or not isinstance(minibatch, int) or minibatch < 1):
        raise ValueError(f"minibatch must be an int >= 1 or None, got {minibatch!r}")
    clip = clip_pair(clip)
    rows = tuple(rows)
    n = rows[1].shape[0]
    reward = torch.as_tensor(reward, dtype=torch.float32).view(-1)
    if reward.numel() != n:
        raise ValueError(f"{reward.numel()} rewards for {n} sequences")
    if weight is not None:
        weight = _check_weight(weight, n, "ppo_update").cpu()
    m = n if minibatch is None else min(int(minibatch), n)
    with_entropy = entropy_coef != 0
    gclip = _GradClip(optimizer, max_grad_norm, "ppo_update")
    history = []
    model.train(bool(train_mode))
    gclip.install()
    try:
        adv = advantages(reward.to(sampler.device), baseline, normalize).cpu()   # the device's arithmetic, as
        if weight is not None:
            adv = adv * weight
        if old_token_logp is None:                                               # reinforce_loss's; checked on the host
            with torch.no_grad():
                old_token_logp = sampler.logp(*rows).token_logp
        for _ in range(epochs):
            if target_kl is not None and history and history[-1]["approx_kl"] > target_kl:
                break
            sums = gnorm = None
            for lo in range(0, n, m):
                hi = min(n, lo + m)
                terms = sampler.ppo_terms(*_row_slice(rows, lo, hi), old_token_logp=old_token_logp[lo:hi],
                                          advantage=adv[lo:hi], clip=clip, prior=prior, entropy=with_entropy)
                optimizer.zero_grad(set_to_none=True)
                loss = ppo_loss(terms, entropy_coef, kl_coef)
                loss.backward()
                gclip.step()
                part = [loss.detach().float() * (hi - lo), terms.surrogate.detach().sum(),
                        terms.clipped.sum().float(), terms.approx_kl.sum(), terms.tokens.sum().float()]
                if with_entropy:
                    part.append(terms.entropy.detach().sum())
                if prior is not None:
                    part += [terms.kl.detach().sum(), terms.prior_logp.sum()]
                if gclip.active:                       # the clipped-update count rides at the end of the sums
                    norm, clipped = (t.to(part[0].device) for t in gclip.norm_and_clipped())
                    gnorm = norm if gnorm is None else torch.maximum(gnorm, norm)
                    part.append(clipped)
                part = torch.stack(part)
                sums = part if sums is None else sums + part
            if gclip.active:
                sums = torch.cat([sums, gnorm.view(1)])
            s = sums.cpu().tolist()
            if gclip.active:
                s, clip_stats = s[:-2], s[-2:]
            tokens = s[4]
            out = dict(loss=s[0] / n, mean_surrogate=s[1] / n, clip_fraction=s[2] / tokens, approx_kl=s[3] / tokens,
                       tokens=int(tokens))
            if with_entropy:
                out["mean_entropy"] = s[5] / tokens
            if prior is not None:
                out["mean_kl"], out["mean_prior_logp"] = s[-2] / tokens, s[-1] / n
            if gclip.active:
                out["clipped_updates"], out["grad_norm"] = int(clip_stats[0]), clip_stats[1]
            if weight is not None:                     # (on the host already: no transfer)
                out["weight_mean"], out["weight_max"] = float(weight.mean()), float(weight.max())
            history.append(out)
    finally:
        gclip.restore()
        model.eval()
    return history
