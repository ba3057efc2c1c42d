"""Timestep-aware step caching (TeaCache, the FLUX recipe): the host side. model_config["step_cache_thresh"] turns it on for the forwards
of one conditioning; the engine (DiTEngine._forward_step_cache) then splits a denoise step into a probe, the blocks and a reuse part, and
this module decides, from one number per forward, which of the two runs.

The rule, per step i of a schedule of n steps. m_i is the image stream's norm1 input of double block 0 in fp32 (lx_ln_modulate_delta),
rel_i = sum |m_i - m_(i-1)| / sum |m_(i-1)| over the whole forward batch, acc a Python float:
    compute  if i == 0, i == n - 1, i is not the previous call's index + 1, or acc + poly(rel_i) >= thresh   -> acc = 0
    skip     otherwise                                                                                      -> acc = acc + poly(rel_i)
poly = numpy.poly1d(coefficients), highest degree first. (A poly(rel_i) that is NaN -- an all-zero m_(i-1) -- computes.)

DEFAULT_COEFFICIENTS is the FLUX.1-dev fit of the TeaCache recipe, quoted from memory and unverifiable offline; it was fitted on a
transformer without a condition stream. (1.0, 0.0) makes poly the identity: the threshold then applies to the raw accumulated distance."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_COEFFICIENTS = (498.651651, -283.781631, 55.8554382, -3.82021401, 0.264230861)


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def step_cache_config(model_config: Optional[Dict]) -> Optional[Tuple[float, Tuple[float, ...]]]:
    """model_config -> (thresh, coefficients), or None when the cache is off (step_cache_thresh absent, None or 0). ValueError for a
    threshold that is not a finite number >= 0, and for coefficients that are not a non-empty sequence of finite numbers (checked whether
    the cache is on or not)."""
    mc = model_config or {}
    coeff = mc.get("step_cache_coefficients")
    if coeff is None:
        coeff = DEFAULT_COEFFICIENTS
    else:
        if isinstance(coeff, (str, bytes)) or not isinstance(coeff, (Sequence, np.ndarray)) or len(coeff) == 0:
            raise ValueError(f'model_config["step_cache_coefficients"] = {coeff!r}: a non-empty sequence of finite numbers, highest degree first')
        if not all(_number(c) and math.isfinite(c) for c in coeff):
            raise ValueError(f'model_config["step_cache_coefficients"] = {coeff!r}: every coefficient must be a finite number')
        coeff = tuple(float(c) for c in coeff)
    thresh = mc.get("step_cache_thresh")
    if thresh is None:
        return None
    if not _number(thresh) or not math.isfinite(thresh) or thresh < 0:
        raise ValueError(f'model_config["step_cache_thresh"] = {thresh!r}: a finite number > 0 (absent, None or 0: off)')
    if thresh == 0:
        return None
    return float(thresh), coeff


def normalise_model_config(mc: Dict) -> Dict:
    """A YAML list of coefficients as the tuple a hashed key can hold (in place; validation is step_cache_config's)."""
    c = mc.get("step_cache_coefficients")
    if isinstance(c, (list, np.ndarray)):
        mc["step_cache_coefficients"] = tuple(float(v) if _number(v) else v for v in c)
    return mc


def decide(i: int, n: int, last: Optional[int], acc: float, rel: Optional[float], thresh: float, poly) -> Tuple[bool, float]:
    """The rule of the module docstring for one step: (compute?, acc after the step). `last`: the previous call's index (None: there was
    none). `rel` is looked at only where nothing else forces the step."""
    if i == 0 or i == n - 1 or last is None or i != last + 1 or rel is None:
        return True, 0.0
    with np.errstate(all="ignore"):                    # (rel = inf: Horner's 0 * inf is the NaN handled below, not a warning)
        total = acc + float(poly(rel))
    if not total < thresh:
        return True, 0.0
    return False, total


class StepCacheState:
    """What the rule remembers between the forwards of one conditioning (acc, the last index) and the report of what it decided."""

    def __init__(self, thresh: float, coefficients: Sequence[float]):
        self.thresh, self.coefficients = float(thresh), tuple(float(c) for c in coefficients)
        self.poly = np.poly1d(self.coefficients)
        self.reset()

    def reset(self) -> None:
        self.acc, self.last = 0.0, None
        self.indices: List[int] = []
        self.computed: List[int] = []
        self.rel: List[Optional[float]] = []
        self.accs: List[float] = []

    def step(self, i: int, n: int, rel: Optional[float]) -> bool:
        """Record step i of n with distance `rel` (None at step 0) -> whether the blocks run."""
        compute, self.acc = decide(i, n, self.last, self.acc, rel, self.thresh, self.poly)
        self.last = i
        self.indices.append(i)
        self.rel.append(None if i == 0 else rel)
        self.accs.append(self.acc)
        if compute:
            self.computed.append(i)
        return compute

    def report(self) -> Dict:
        return dict(steps=len(self.indices), indices=list(self.indices), computed=list(self.computed), rel=list(self.rel), acc=list(self.accs),
                    thresh=self.thresh, coefficients=self.coefficients)
