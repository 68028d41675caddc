"""model_type -> forward function (reference Model/forward_propagation1.py:4-48): builds the
masks from the batch (on the batch's device, no host round trip; the decoder's self-attention mask straight from
the token ids) and calls model.forward by keyword exactly like the reference.

skip_ignored (an extension, default False = the reference's behaviour): tell the model which decoder rows the
reference's loss looks at -- `ys = trg[:, 1:] != pad` (Train/trainer1.py:21-22,97: cross-entropy with
ignore_index = pad) -- so that it does not compute the others (56 % of the decoder rows at MOSES-like lengths).  Loss
and every gradient are unchanged; the logits of the ignored rows are not the reference's (nothing reads them).  The
trainer (Train/trainer1.run_epoch) and bench.py switch it on; a caller that wants every logit leaves it off."""
from .. import ops
from .modules import get_src_mask, get_trg_mask


def _trg_mask(trg_in, pad_id, use_cond2dec, dconds=None):
    """get_trg_mask; on the GPU and without cond2dec its uint8 form comes from the token ids in one launch
    (ops.trg_mask_u8) instead of the int64 [B,T,T] tensor -- the model only asks whether an entry is nonzero."""
    if trg_in.is_cuda and not use_cond2dec and trg_in.dim() == 2 and trg_in.stride(1) == 1:
        return ops.trg_mask_u8(trg_in, pad_id)
    return get_trg_mask(trg_in, pad_id, use_cond2dec, dconds)


def _masks(batch, pad_id, use_cond2dec, skip_ignored, conditioned):
    trg_in = batch["trg"][:, :-1]
    rows = batch["trg"][:, 1:] != pad_id if skip_ignored else None     # (the model's row planner decides their use)
    if conditioned:
        return (trg_in, get_src_mask(batch["src"], pad_id, batch["econds"]),
                _trg_mask(trg_in, pad_id, use_cond2dec, batch["dconds"]), rows)
    return trg_in, get_src_mask(batch["src"], pad_id), _trg_mask(trg_in, pad_id, use_cond2dec), rows


def latent_live_rows(model_type, batch, pad_id):
    """bool [B, 1, Le]: the latent rows (mu, log_var [B, Le, D]) that stand for a real source position or a condition
    -- the encoder's key mask of _masks, the one mask rule.  The KL controls of Train/trainer1 and the latent report
    count these rows only."""
    if forward_propagation[model_type] is _conditioned:
        return get_src_mask(batch["src"], pad_id, batch["econds"])
    return get_src_mask(batch["src"], pad_id)


def _held(batch, conditioned):
    return (batch["src"], batch["trg"]) + ((batch["econds"], batch["dconds"]) if conditioned else ())


def prefetch(model_type, model, batch, pad_id, use_cond2dec, skip_ignored=False):
    """Queue, NOW, the masks and the row maps of a batch that the NEXT call of forward_propagation[model_type] will get
    (same arguments).  The trainer calls it between a step's forward and its backward: the maps' one device->host
    read-back then completes while that backward runs, and the next step's forward is queued without the host waiting
    for the device (engine.RowPlan).  Purely an optimisation: the announcement holds the batch's tensors, and a forward
    takes it only for those very tensor objects (`is`) at the versions they had here -- any other batch, a view of
    these tensors, or a batch modified since is handled exactly as if nothing had been announced.  GPU batches and
    models with plan_ahead only; a no-op otherwise."""
    inner = getattr(model, "module", model)
    if not (hasattr(inner, "plan_ahead") and batch["src"].is_cuda):
        return
    conditioned = forward_propagation[model_type] is _conditioned
    held = _held(batch, conditioned)
    trg_in, src_mask, trg_mask, rows = _masks(batch, pad_id, use_cond2dec, skip_ignored, conditioned)
    inner._gct_ahead = (held, tuple(t._version for t in held), (pad_id, bool(use_cond2dec), bool(skip_ignored)),
                        (src_mask, trg_mask, rows, inner.plan_ahead(src_mask, trg_mask, rows, trg_in)))


def forget_announcement(model):
    """Drop whatever prefetch() announced (run_epoch, at its start)."""
    getattr(model, "module", model)._gct_ahead = None


def _ahead(model, batch, pad_id, use_cond2dec, skip_ignored, conditioned):
    inner = getattr(model, "module", model)
    got = getattr(inner, "_gct_ahead", None)
    if got is None:
        return None
    inner._gct_ahead = None
    held, versions, flags, ahead = got
    now = _held(batch, conditioned)
    same = (len(now) == len(held) and all(a is b and a._version == v for a, b, v in zip(now, held, versions))
            and flags == (pad_id, bool(use_cond2dec), bool(skip_ignored)))
    return ahead if same else None


def _call(model, batch, pad_id, use_cond2dec, skip_ignored, conditioned):
    ahead = _ahead(model, batch, pad_id, use_cond2dec, skip_ignored, conditioned)
    kw = {}
    if ahead is not None:
        src_mask, trg_mask, rows, kw["_plan_ahead"] = ahead
        trg_in = batch["trg"][:, :-1]
    else:
        trg_in, src_mask, trg_mask, rows = _masks(batch, pad_id, use_cond2dec, skip_ignored, conditioned)
    if rows is not None:
        kw["loss_rows"] = rows
    if conditioned:
        kw.update(econds=batch["econds"], dconds=batch["dconds"])
    return model.forward(src=batch["src"], trg=trg_in, src_mask=src_mask, trg_mask=trg_mask, **kw)


def _plain(model, batch, pad_id, use_cond2dec, skip_ignored=False):
    return _call(model, batch, pad_id, use_cond2dec, skip_ignored, False)


def _conditioned(model, batch, pad_id, use_cond2dec, skip_ignored=False):
    return _call(model, batch, pad_id, use_cond2dec, skip_ignored, True)


forward_propagation = {
    "vaetf": _plain,
    "scavaetf": _plain,
    "pvaetf": _conditioned,
    "pscavaetf": _conditioned,
}
