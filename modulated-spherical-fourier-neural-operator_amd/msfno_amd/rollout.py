"""Checkpoint loading and the autoregressive rollout driver.

* ``load_checkpoint`` follows MSFNO/Models/sfno/model.py:206-271 (``load_model``):
  optional ``"model_state"`` wrapper, the ``drop_vars`` filter, the DDP
  ``"module."`` prefix strip (and its ``"ged"`` entry), strict load first and
  ``strict=False`` on failure (the ECMWF weights lack the SHT buffers
  ``trans_down.weights`` / ``itrans_up.pct``).  Files are read with
  ``torch.load(weights_only=True)`` — nothing in a checkpoint is executed.
* ``load_filmed_checkpoint`` follows model.py:917-1033 (``FourCastNetv2_filmed.
  load_model``): the same SFNO load, the ``--retrain-film`` skip list, the
  FiLM-generator checkpoint merge (``"film_gen."`` prefix) and the freeze rule.
* ``Rollout`` is ``running()`` (model.py:289-372) without the GRIB I/O: the
  state stays on the GPU between 6 h steps (the reference copies every output
  to the host before writing it), ``normalise`` is model.py:273-279, and one
  step can be captured as a HIP graph and replayed.
"""
from __future__ import annotations

import warnings

import torch

DROP_VARS = ("module.norm.weight", "module.norm.bias")  # model.py:216


def _read(checkpoint, map_location):
    if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "read"):
        checkpoint = torch.load(checkpoint, map_location=map_location, weights_only=True)
    return checkpoint


def _load_with_fallback(module, weights, what="state dict"):
    """Strict load, then ``strict=False`` on a RuntimeError (model.py:240-256,
    956-964).  Returns whether the strict load succeeded."""
    try:
        module.load_state_dict(weights)
        return True
    except RuntimeError as e:
        warnings.warn(f"{what}: loading with strict=False ({str(e).splitlines()[0]})",
                      stacklevel=3)
        module.load_state_dict(weights, strict=False)
        return False


def _sfno_weights(checkpoint, skip=None):
    """model_state wrapper, drop_vars, the DDP "module." prefix and its "ged"
    entry (model.py:216-239, 927-955); ``skip(name)`` drops a key (the
    retrain_film rule, model.py:952 / 969)."""
    weights = checkpoint["model_state"] if "model_state" in checkpoint else checkpoint
    weights = {k: v for k, v in weights.items() if k not in DROP_VARS}
    prefixed = bool(weights) and next(iter(weights)).startswith("module.")
    out = {}
    for k, v in weights.items():
        name = k[7:] if prefixed else k
        if skip is not None and skip(name):
            continue
        if prefixed and name == "ged":
            continue
        out[name] = v
    return out


def load_checkpoint(model, checkpoint, map_location="cpu"):
    """Load a reference checkpoint (path or already-loaded dict) into ``model``
    (FourCastNetv2.load_model, model.py:207-271).  Returns ``(model, strict)``
    where ``strict`` tells whether the strict load succeeded."""
    weights = _sfno_weights(_read(checkpoint, map_location))
    strict = _load_with_fallback(model, weights)
    model.eval()
    model.zero_grad()
    return model, strict


def retrain_film_layers(film_layers):
    """The trainable-name substrings of ``--retrain-film`` (model.py:923): the FiLM
    generator, the decoder and the last ``film_layers`` blocks, counted down from
    block 11 as the reference writes it (a 12-block network)."""
    return ["film_gen", "decoder"] + ["blocks." + str(11 - i) for i in range(film_layers)]


def load_filmed_checkpoint(model, checkpoint, film_checkpoint=None, retrain_film=False,
                           film_layers=1, resume_checkpoint=None, map_location="cpu"):
    """FourCastNetv2_filmed.load_model (model.py:917-1033) for a
    FourierNeuralOperatorNet_Filmed:

    * SFNO weights as ``load_checkpoint``; with ``retrain_film`` (and no
      ``resume_checkpoint``) every key containing one of
      ``retrain_film_layers(film_layers)`` is skipped (model.py:952, 969), so
      those layers keep their fresh initialisation;
    * the FiLM-generator checkpoint's ``model_state`` is prefixed with
      ``"film_gen."`` unless it already is, and loaded into ``model.film_gen``
      (model.py:983-1003); if that load fails the reference retries with the raw
      checkpoint dict and ``strict=False``, which loads nothing: reproduced, with a
      warning;
    * freeze (model.py:1016-1023): with ``retrain_film`` every parameter outside
      those layers gets ``requires_grad=False``; otherwise every parameter whose
      name lacks ``"film_gen"``.

    Returns ``(model, strict)`` for the SFNO load."""
    model.zero_grad()
    grad_layers = retrain_film_layers(film_layers) if retrain_film else None

    def skip(name):
        return (retrain_film and resume_checkpoint is None
                and any(layer in name for layer in grad_layers))

    weights = _sfno_weights(_read(checkpoint, map_location), skip)
    strict = _load_with_fallback(model, weights, "SFNO weights")
    if film_checkpoint is not None:
        ck = _read(film_checkpoint, map_location)
        film_weights = ck["model_state"]
        if not next(iter(film_weights)).startswith("film_gen."):
            film_weights = {"film_gen." + k: v for k, v in film_weights.items()}
        if model.film_gen is None:
            raise ValueError("a FiLM-generator checkpoint needs model.film_gen")
        try:
            model.film_gen.load_state_dict(film_weights)
        except RuntimeError as e:
            warnings.warn("Film Gen: loading with strict=False, as the reference does "
                          f"(model.py:1003; nothing is loaded): {str(e).splitlines()[0]}",
                          stacklevel=2)
            model.film_gen.load_state_dict({k: v for k, v in ck.items()
                                            if isinstance(v, torch.Tensor)}, strict=False)
    for name, param in model.named_parameters():
        if retrain_film:
            if not any(layer in name for layer in grad_layers):
                param.requires_grad = False
        elif "film_gen" not in name:
            param.requires_grad = False
    model.eval()
    model.zero_grad()
    return model, strict


def _whole_fields_only(model, regrid):
    if regrid is not None and getattr(model, "world", 1) > 1:
        raise NotImplementedError(
            "regrid= maps whole fields; on a latitude-band rank the rows of a destination "
            "cell's band lie on the neighbouring ranks too, and band-sharded regridding is "
            "not implemented")


class Rollout:
    """On-device autoregressive stepping of a FourierNeuralOperatorNet[_Filmed], or
    of one rank's ``LatBandNet`` (the multi-GPU form of config 5: every rank steps
    its own latitude rows; x0 is then ``shard.take(x0)`` and the outputs are the
    rank's rows).

    ``means`` / ``stds`` broadcast against the (B, C, H, W) state (the
    reference's global statistics, model.py:190-204: per channel, so they apply to
    a rank's rows unchanged).  ``film`` is the FiLM modulation passed to Filmed
    networks every step (or None).  A sharded network with more than one rank is
    captured too when its exchanges run on RCCL (a ``TorchComm`` over the nccl
    backend: the collectives are recorded into the graph, model.py:327-331's
    per-step cost without the host launches); over gloo (host collectives) it steps
    eagerly, and a capture that fails on any rank makes every rank step eagerly
    (``TorchComm.all_agree``).

    ``noise`` is a ``harmonics.SphericalAR1`` whose ``lead`` is the state's (B, C): every
    step is then ``x <- model(x) + noise.step()`` in normalised units, in the eager loop
    and inside the captured graph alike (the process keeps its draw counter on the device,
    so every replay draws anew).  ``run`` does not reset the process."""

    def __init__(self, model, means=None, stds=None, film=None, scale=1.0, graph=True,
                 noise=None):
        if noise is not None and getattr(model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout with noise steps whole fields; band-sharded noise is not "
                "implemented (the stream is defined per (field, l, m), so a band rank can "
                "generate its share)")
        self.noise = noise
        self.model = model
        self.means, self.stds = means, stds
        self.film, self.scale = film, scale
        comm = getattr(model, "comm", None)
        device_comm = comm is not None and not getattr(comm, "host", True)
        # capture-or-eager must be one decision for all ranks (all_agree); a multi-rank
        # comm that cannot agree steps eagerly on every rank
        agreeable = device_comm and callable(getattr(comm, "all_agree", None))
        self.use_graph = graph and (getattr(model, "world", 1) == 1 or agreeable)
        self._graph = None

    def normalise(self, data, reverse=False):
        """model.py:273-279."""
        if self.means is None:
            return data
        if reverse:
            return data * self.stds + self.means
        return (data - self.means) / self.stds

    def _step(self, x):
        y = self.model(x) if self.film is None else self.model(x, self.film, self.scale)
        if self.noise is None:
            return y
        return y + self.noise.step()

    def _capture(self, x):
        self._state = x.clone()
        # the warm-up must not advance the noise process
        snap = None if self.noise is None else self.noise.snapshot()
        self._step(self._state)  # warm-up: plans, descriptors, allocator pools
        if snap is not None:
            self.noise.restore(snap)
        quiesce = getattr(getattr(self.model, "comm", None), "quiesce", None)
        if callable(quiesce):
            quiesce()  # no RCCL work of the warm-up left for the watchdog to poll
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._out = self._step(self._state)
        self._graph = g

    @torch.no_grad()
    def run(self, x0, steps, normalised_input=False):
        """Yields (step_index, denormalised output on the device) for ``steps``
        6 h steps starting from ``x0`` (raw fields unless ``normalised_input``)."""
        x = x0 if normalised_input else self.normalise(x0)
        x = x.contiguous()
        if self.noise is not None and tuple(x.shape[:2]) != tuple(self.noise.lead):
            raise ValueError(f"the noise process has lead {tuple(self.noise.lead)}, the state "
                             f"is {tuple(x.shape)}")
        if self.use_graph and x.is_cuda and (self._graph is None or self._state.shape != x.shape):
            if getattr(self.model, "world", 1) == 1:
                self._capture(x)
            else:
                # capture-or-eager is decided by all ranks together: a rank whose
                # capture failed (a collective the backend cannot record) must not step
                # eagerly while its peers replay recorded collectives
                ok = True
                try:
                    self._capture(x)
                except RuntimeError:
                    ok = False
                    torch.cuda.synchronize()
                ok = self.model.comm.all_agree(ok)
                if not ok:
                    self._graph = None
                    self.use_graph = False
        if self.use_graph and x.is_cuda:
            self._state.copy_(x)
            for i in range(steps):
                self._graph.replay()
                # the graph's output buffer is overwritten by the next replay: hand the
                # caller a tensor of its own (normalise(reverse) already makes one)
                y = self.normalise(self._out, reverse=True)
                yield i, (y.clone() if y is self._out else y)
                self._state.copy_(self._out)
        else:
            for i in range(steps):
                x = self._step(x)
                yield i, self.normalise(x, reverse=True)

    def verify(self, x0, truths, steps, every=1, weights="uniform", normalised_input=False,
               verifier=None, regrid=None, regions=None, skip_nan=False):
        """Score a rollout on the device (model.py:737-758, train.py:533-583 without the
        per-step copy to the host): ``run(x0, steps)`` with every step ``i`` where
        ``i % every == 0`` (``every = validation_step_skip + 1``, train.py:551) scored
        against the next item of ``truths``: ``tar``, ``(tar, clim)`` or
        ``(tar, clim, clim_slab)``, raw fields as ``verification.field_sums`` takes them
        (host tensors are copied without blocking).  Returns ``verification.Scores`` of
        (n_scored, B, C) tensors under ``weights`` (``verification.Verifier``).  Pass a
        ``verifier`` of your own to keep the raw sums (``verifier.sums``) or to reuse its
        buffers; its weights then apply.  With ``regrid`` (a ``regrid.Regridder`` from the
        model's grid) every scored output goes through it first: truths are then given on the
        destination grid, the default verifier is built for the destination shape and a
        ``weights`` name means the destination grid's latitudes.  With ``regions`` (a
        ``regions.Regions`` of the scored grid: the destination grid under ``regrid``) the
        default verifier is a ``verification.RegionalVerifier`` and the scores are
        (n_scored, B, C, R), one column per region; ``skip_nan`` then leaves out the pixels
        whose truth or climatology is NaN."""
        from . import verification as V
        _whole_fields_only(self.model, regrid)
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.verify scores whole fields; on a latitude-band rank call "
                "verification.field_sums on the rank's rows with w[rows] and "
                "clim[..., rows, :], all-reduce the (B, C, 6) sums over the ranks, then "
                "verification.finish with the whole grid's w; for regions, "
                "verification.region_sums with regions.rows(rows), all-reduce the "
                "(B, C, R, 7) sums, then verification.finish_regions")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        if skip_nan and regions is None and verifier is None:
            raise ValueError("skip_nan needs regions (regions.Regions.boxes(grid, {'global': "
                             "(None, None, None, None)}) for the whole grid)")
        n_scored = (steps + every - 1) // every
        B, C, H, W = x0.shape
        if regrid is not None:
            H, W = regrid.out_shape
        if regions is not None:
            if tuple(getattr(regions, "shape", ())) != (H, W):
                raise ValueError(f"the regions are of a {getattr(regions, 'shape', None)} grid, "
                                 f"the scored fields are {(H, W)}")
            if verifier is not None and getattr(verifier, "regions", None) is not regions:
                raise ValueError("pass regions or a verifier built on them, not two that "
                                 "differ")
        if verifier is None and regions is not None:
            verifier = V.RegionalVerifier(weights, regions, n_scored, B, C, skip_nan=skip_nan,
                                          device=x0.device)
        elif verifier is None:
            verifier = V.Verifier(weights, H, W, n_scored, B, C, device=x0.device)
        elif verifier.sums.shape[0] < n_scored:
            raise ValueError(f"verifier has {verifier.sums.shape[0]} slots, {n_scored} needed")
        truths = iter(truths)
        for i, y in self.run(x0, steps, normalised_input=normalised_input):
            if i % every:
                continue
            try:
                item = next(truths)
            except StopIteration:
                raise ValueError(f"truths ran out at step {i}: {n_scored} scored steps need "
                                 "one item each") from None
            if isinstance(item, torch.Tensor):
                item = (item,)
            verifier.update(i // every, y if regrid is None else regrid(y), *item)
        return verifier.scores()

    def verify_maps(self, x0, truths, steps, every=1, maps=None, normalised_input=False,
                    regrid=None, skip_nan=False):
        """Score maps of a rollout on the device: runs as ``verify`` does, and every scored
        step ``i`` (``i % every == 0``) folds the batch of cases into ``maps[i // every]``,
        an ``ErrorMaps`` of a ``timestats.LeadTimeMaps``: per-pixel bias, RMSE, MAE and ACC
        per lead time.  Returns ``maps``; pass the same ``maps`` for the next batch of
        initial dates.  ``truths`` are items as in ``verify``; a climatology in an item needs
        maps built with ``anomalies=True`` (the default maps are, iff the first item has one),
        and every slab of it is read (no -1 in a ``clim_slab``).  ``regrid`` as in ``verify``:
        maps and truths are then of the destination grid.  With ``skip_nan`` a case is left
        out of a pixel where its truth or climatology is NaN.

        Memory: 3 planes and the count per lead time, 8 with anomalies; at 73 x 721 x 1440 a
        plane is 303 MB and a lead time with anomalies 2.7 GB, so ``regrid=`` to 1.5 degrees
        or a channel subset is the way to keep 40 lead times."""
        from . import timestats as T
        _whole_fields_only(self.model, regrid)
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.verify_maps maps whole fields; on a latitude-band rank keep a "
                "timestats.LeadTimeMaps of the rank's own rows and update it with the rank's "
                "rows of the output, the truth and the climatology: the maps are per pixel, "
                "there is nothing to reduce")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        n_scored = (steps + every - 1) // every
        B, C, H, W = x0.shape
        if regrid is not None:
            H, W = regrid.out_shape
        if maps is not None:
            if len(maps) < n_scored:
                raise ValueError(f"maps has {len(maps)} lead times, {n_scored} needed")
            if tuple(maps.shape) != (C, H, W):
                raise ValueError(f"maps are of {tuple(maps.shape)} fields, the scored fields "
                                 f"are {(C, H, W)}")
        truths = iter(truths)
        for i, y in self.run(x0, steps, normalised_input=normalised_input):
            if i % every:
                continue
            try:
                item = next(truths)
            except StopIteration:
                raise ValueError(f"truths ran out at step {i}: {n_scored} scored steps need "
                                 "one item each") from None
            if isinstance(item, torch.Tensor):
                item = (item,)
            if maps is None:
                maps = T.LeadTimeMaps(n_scored, C, H, W, anomalies=len(item) > 1,
                                      device=x0.device)
            maps[i // every].update(y if regrid is None else regrid(y), *item,
                                    skip_nan=skip_nan)
        return maps

    def statistics(self, x0, steps, stats, every=1, normalised_input=False, regrid=None):
        """The time mean and variability of a rollout: folds every output ``i`` of
        ``run(x0, steps)`` where ``i % every == 0`` into ``stats``, a
        ``timestats.FieldStats`` of the output's (C, H, W) (of the destination grid under
        ``regrid``), batch elements in order.  Returns ``stats``; pass it again to go on.
        At 73 x 721 x 1440 a plane is 303 MB and a ``FieldStats`` is 2 planes and the count
        (4 with ``minmax``)."""
        _whole_fields_only(self.model, regrid)
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.statistics folds whole fields; on a latitude-band rank keep a "
                "timestats.FieldStats of the rank's own rows and update it with the rank's "
                "rows of every output: the statistics are per pixel, there is nothing to "
                "reduce")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        for i, y in self.run(x0, steps, normalised_input=normalised_input):
            if i % every == 0:
                stats.update(y if regrid is None else regrid(y))
        return stats

    def verify_ensemble(self, x0, truths, steps, every=1, weights="uniform",
                        normalised_input=False, verifier=None, regrid=None):
        """Score an ensemble rollout on the device: the batch of ``x0`` (M, C, H, W) is the
        M members of one case (``self.film`` may differ per member), stepped together by
        ``run(x0, steps)``; every step ``i`` where ``i % every == 0`` is scored against the
        next item of ``truths``, a raw field (C, H, W) or (1, C, H, W) (a host tensor is
        copied without blocking), exactly as ``verify`` pairs them.  The scored output is
        viewed as (M, 1, C, H, W) without a copy.  Returns ``ensemble.EnsembleScores`` of
        (n_scored, 1, C) tensors and the (n_scored, 1, C, M + 1) rank histograms under
        ``weights`` (``ensemble.EnsembleVerifier``).  Pass a ``verifier`` of your own (built
        with B = 1) to keep the raw sums or to reuse its buffers; its weights then apply.
        ``regrid`` as in ``verify``: the members are regridded before they are scored, and
        truths, verifier and weights are those of the destination grid."""
        from . import ensemble as E
        _whole_fields_only(self.model, regrid)
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.verify_ensemble scores whole fields; on a latitude-band rank call "
                "ensemble.ensemble_sums on the rank's rows with w[rows], all-reduce the "
                "(B, C, 5) sums and the (B, C, M + 1) rank counts over the ranks, then "
                "ensemble.finish with the whole grid's w")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        if x0.dim() != 4:
            raise ValueError(f"x0 must be (M, C, H, W), got {tuple(x0.shape)}")
        M, C, H, W = x0.shape
        if regrid is not None:
            H, W = regrid.out_shape
        n_scored = (steps + every - 1) // every
        if verifier is None:
            verifier = E.EnsembleVerifier(weights, H, W, n_scored, M, 1, C, device=x0.device)
        elif verifier.sums.shape[0] < n_scored:
            raise ValueError(f"verifier has {verifier.sums.shape[0]} slots, {n_scored} needed")
        truths = iter(truths)
        for i, y in self.run(x0, steps, normalised_input=normalised_input):
            if i % every:
                continue
            try:
                tar = next(truths)
            except StopIteration:
                raise ValueError(f"truths ran out at step {i}: {n_scored} scored steps need "
                                 "one item each") from None
            if tuple(tar.shape) not in ((C, H, W), (1, C, H, W)):
                raise ValueError(f"a truth must be (C, H, W) or (1, C, H, W) = {(C, H, W)}, "
                                 f"got {tuple(tar.shape)}")
            if regrid is not None:
                y = regrid(y)
            verifier.update(i // every, y.contiguous().view(M, 1, C, H, W),
                            tar.reshape(1, C, H, W))
        return verifier.scores()

    def ensemble_products(self, x0, steps, every=1, normalised_input=False, **products_kwargs):
        """An iterator of ``(step, ensemble.EnsembleProducts)`` for every step ``i`` of an ensemble
        rollout where ``i % every == 0``: the batch of ``x0`` (M, C, H, W) is the M members
        of one case, stepped together by ``run(x0, steps)``, and the products are those of
        the denormalised output, viewed as (M, 1, C, H, W) without a copy, so the maps are
        (1, C, H, W) (quantiles and prob (n, 1, C, H, W)).  ``products_kwargs`` go to
        ``ensemble.products`` (``quantiles``, ``thresholds``, ``mean``, ``std``,
        ``minmax``)."""
        from . import ensemble as E
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.ensemble_products maps whole fields; on a latitude-band rank call "
                "ensemble.products on the rank's rows: the maps are row-local, nothing is "
                "exchanged")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        if x0.dim() != 4:
            raise ValueError(f"x0 must be (M, C, H, W), got {tuple(x0.shape)}")
        M, C, H, W = x0.shape

        def maps():
            for i, y in self.run(x0, steps, normalised_input=normalised_input):
                if i % every == 0:
                    yield i, E.products(y.contiguous().view(M, 1, C, H, W), **products_kwargs)

        return maps()  # the refusals above are raised by the call, not by the first next()

    def export(self, x0, steps, writer, every=1, normalised_input=False, regrid=None):
        """Hand every step ``i`` of ``run(x0, steps)`` where ``i % every == 0`` to
        ``writer.put(i, y)`` (an ``export.ForecastWriter`` made for the shape of ``x0``): the
        denormalised output is subset and packed on the device and copied to the host under
        the following steps.  Does not flush, so that a writer can be kept across cases: call
        ``writer.flush()`` (or leave its ``with`` block) to receive what is still in flight.
        With ``regrid`` (a ``regrid.Regridder`` from the model's grid) the writer is one made
        for the destination shape and receives the regridded field.
        Returns the number of steps put."""
        _whole_fields_only(self.model, regrid)
        if getattr(self.model, "world", 1) > 1:
            raise NotImplementedError(
                "Rollout.export packs whole fields; on a latitude-band rank the range of a "
                "field spans the ranks: min / max of the rank's rows would have to be "
                "all-reduced before the pack pass, which is not implemented")
        if steps < 1 or every < 1:
            raise ValueError("steps and every must be >= 1")
        n = 0
        for i, y in self.run(x0, steps, normalised_input=normalised_input):
            if i % every == 0:
                writer.put(i, y if regrid is None else regrid(y))
                n += 1
        return n
