"""Policy-gradient fine-tuning on what the sampler drew: the per-molecule objective the ELBO trainer (trainer1.py) does
not have.  `reinforce_loss` is the REINFORCE surrogate over differentiable sequence log-likelihoods
(decode.sequence_logp -> gct_seq_logp_bwd), `reinforce_step` one update of a sampler's model on rows it decoded:

    out = sampler.sample_smiles(..., return_rows=True)          # ..., DecodedRows
    reward = torch.tensor([score(s) for s in out[0]])           # any per-molecule number
    stats = reinforce_step(sampler, optimizer, out[-1], reward)

Reward-weighted likelihood, hill-climbing on the best k of a batch and any other per-molecule loss are functions of
`sampler.logp(*rows).logp` in the same way.  Not covered: FlatDataParallel fine-tuning, a prior-KL term (a
caller composes it from decode.score_tokens on a second, frozen model), importance ratios, beam rows."""
import torch


def reinforce_loss(logp, reward, baseline="mean"):
    """-((reward - b) * logp).sum() / n over the n sequences of a batch: minimising it raises the log-likelihood of the
    sequences whose reward lies above the baseline b and lowers that of the others.  logp [n] (with a graph), reward [n]
    numbers (no gradient flows into them); baseline "mean": the batch mean of the reward, a float or a tensor
    (broadcast against reward): that value, None: 0."""
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
    return -((reward - b) * logp.view(-1)).sum() / logp.numel()


def reinforce_step(sampler, optimizer, rows, reward, baseline="mean"):
    """One policy-gradient update of sampler.model on the decoded rows `rows` (a DecodedRows, or any argument tuple of
    Sampling.logp) with one reward per row: model.train(), sampler.logp(*rows), optimizer.zero_grad(set_to_none=True),
    reinforce_loss -> backward -> optimizer.step(), model.eval().  Returns dict(loss, mean_reward, mean_logp, tokens),
    Python numbers read in ONE transfer (tokens: the scored tokens of the batch).

    The model runs in training mode, so its dropout is live in this forward: the logp of the step is not the eval-mode
    number `with_logp` reported for the same rows (build the model with dropout 0 where the two must agree).

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
    reward = torch.as_tensor(reward, dtype=torch.float32)
    model.train()
    try:
        scores = sampler.logp(*rows)
        optimizer.zero_grad(set_to_none=True)
        loss = reinforce_loss(scores.logp, reward, baseline)
        loss.backward()
        optimizer.step()
    finally:
        model.eval()
    dev = scores.logp.device
    stats = torch.stack([loss.detach().float(), reward.to(dev).mean(), scores.logp.detach().mean(),
                         scores.tokens.sum().float()]).cpu().tolist()
    return dict(loss=stats[0], mean_reward=stats[1], mean_logp=stats[2], tokens=int(stats[3]))
