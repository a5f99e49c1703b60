"""The step health record read back: per stored tensor of a training step its range, its non-finite counts and an exponent
histogram (option "health" of include/m2t.h, which defines a row; csrc/k_health.hip writes it), and what an FP8 plan would have to
know about that histogram.  Reading a report is the one host synchronisation of the feature: the step itself never reads.

The rows are named by the library (m2t_plan_query "health_rows" / "health_name:<i>" / "health_phase:<i>"); no name table lives here.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

SLOTS = 72
BINS = 64
BIN_OFFSET = 42                  # bin = clamp(floor(log2 |x|), -41, 20) + 42 for finite non-zero elements
PHASES = ("forward", "backward")
# format: (binade of the largest finite value, binade of the smallest normal, binade of the smallest subnormal)
# e4m3 (OCP FP8, the gfx950 matrix cores' E4M3FN): max 448 = 1.75 * 2^8, min normal 2^-6, min subnormal 2^-9
# e5m2:                                            max 57344 = 1.75 * 2^15, min normal 2^-14, min subnormal 2^-16
FP8_FORMATS = {"e4m3": (8, -6, -9), "e5m2": (15, -14, -16)}


class HealthRow:
    """One row of the record: ``n, nonfinite, nan, absmax, mean, rms, zeros, min_nonzero, hist`` (+ ``name``, ``phase``, ``sum``,
    ``sumsq``).  mean and rms run over the finite elements (NaN when there are none)."""

    __slots__ = ("name", "phase", "n", "nonfinite", "nan", "absmax", "sum", "sumsq", "mean", "rms", "zeros", "min_nonzero", "hist")

    def __init__(self, name: str, phase: str, rec):
        rec = np.asarray(rec, dtype=np.float64)
        if rec.shape != (SLOTS,):
            raise ValueError(f"a health row is {SLOTS} doubles, got shape {rec.shape}")
        self.name, self.phase = name, phase
        self.n, self.nonfinite, self.nan = int(rec[0]), int(rec[1]), int(rec[2])
        self.absmax, self.sum, self.sumsq = float(rec[3]), float(rec[4]), float(rec[5])
        self.zeros, self.min_nonzero = int(rec[6]), float(rec[7])
        self.hist = rec[8:].astype(np.int64)
        finite = self.n - self.nonfinite
        self.mean = self.sum / finite if finite > 0 else math.nan
        self.rms = math.sqrt(self.sumsq / finite) if finite > 0 else math.nan

    def __repr__(self):
        return (f"HealthRow({self.name!r}, {self.phase}, n={self.n}, nonfinite={self.nonfinite}, nan={self.nan}, absmax={self.absmax:.4g}, "
                f"mean={self.mean:.4g}, rms={self.rms:.4g}, zeros={self.zeros}, min_nonzero={self.min_nonzero:.4g})")


def fp8_shares(hist, fmt: str = "e4m3") -> Optional[Dict[str, float]]:
    """What one per-tensor scale leaves of a tensor in FP8, from the 64-bin exponent histogram ALONE.

    Binade arithmetic.  Bin k (1 .. 62) holds the finite non-zero elements with floor(log2 |x|) = k - 42 (the two end bins also
    hold everything beyond them).  Let e_max be the binade of the highest occupied bin: absmax lies in [2^e_max, 2^(e_max + 1)).
    The scale is the power of two 2^(E - e_max), E = floor(log2 max_finite) of the format (8 for e4m3, 15 for e5m2): it puts
    absmax's binade on the format's top binade -- all a histogram can know; the exact scale max_finite / absmax differs from it by
    less than one binade.  An element of binade e then lands in binade e' = e + E - e_max and is
      normal     when e' >= the binade of the smallest normal (-6 / -14),
      subnormal  when it is below that and >= the binade of the smallest subnormal (-9 / -16): it keeps 3 .. 1 (e4m3) or 2 .. 1
                 (e5m2) significant bits,
      flush      below: it rounds to zero or to the smallest subnormal.
    Returns the three shares of the finite non-zero elements, ``binades`` (occupied span, top to bottom) and ``e_max``; None for a
    tensor without a finite non-zero element."""
    if fmt not in FP8_FORMATS:
        raise ValueError(f"fp8_report: fmt must be one of {sorted(FP8_FORMATS)}, got {fmt!r}")
    top, lo_normal, lo_sub = FP8_FORMATS[fmt]
    h = np.asarray(hist, dtype=np.int64)
    if h.shape != (BINS,):
        raise ValueError(f"a health histogram has {BINS} bins, got shape {h.shape}")
    body = h[1:BINS - 1]
    total = int(body.sum())
    if total == 0:
        return None
    occupied = np.nonzero(body)[0] + 1
    e_max, e_min = int(occupied[-1]) - BIN_OFFSET, int(occupied[0]) - BIN_OFFSET
    landed = np.arange(1, BINS - 1) - BIN_OFFSET + (top - e_max)
    normal = int(body[landed >= lo_normal].sum())
    sub = int(body[(landed < lo_normal) & (landed >= lo_sub)].sum())
    return {"normal": normal / total, "subnormal": sub / total, "flush": (total - normal - sub) / total,
            "binades": e_max - e_min + 1, "e_max": e_max}


class HealthReport:
    """The record of one plan at the moment it was read: rows by name (``report["b0.xc"]``, ``"sr"``, ``"grads"``), in row order
    when iterated; ``forward_passes`` / ``backward_passes`` recorded so far."""

    def __init__(self, names: List[str], phases: List[int], record):
        rec = np.asarray(record, dtype=np.float64).reshape(-1, SLOTS)
        if rec.shape[0] != 1 + len(names) or len(phases) != len(names):
            raise ValueError(f"health record of {rec.shape[0]} rows for {len(names)} names")
        self.record = rec
        self.forward_passes, self.backward_passes = int(rec[0, 0]), int(rec[0, 1])
        self._first = (int(rec[0, 2]), int(rec[0, 3]))
        self.rows = [HealthRow(n, PHASES[p], rec[1 + i]) for i, (n, p) in enumerate(zip(names, phases))]
        self._by_name = {r.name: r for r in self.rows}

    @classmethod
    def from_plan(cls, plan) -> "HealthReport":
        """Reads ``ws:health`` of a Plan made with ``options={"health": 1 or 2}`` (one device-to-host copy: synchronises)."""
        from . import _lib
        rows = plan.query("health_rows")
        if rows <= 0:
            raise _lib.M2TError("this plan keeps no health record (option \"health\" is 0): M2Trans.track_health() / "
                                "TrainStep(track_health=K) before the plan is made")
        lib = _lib.load()
        names, phases = [], []
        for i in range(rows):
            if plan.query(f"health_name:{i}") < 0:
                raise _lib.M2TError(f"health row {i} has no name")
            names.append(lib.m2t_last_error_string().decode())
            phases.append(plan.query(f"health_phase:{i}"))
        import torch
        rec = plan.ws_tensor("health", (1 + rows, SLOTS), torch.float64).cpu().numpy()
        return cls(names, phases, rec)

    def __getitem__(self, name: str) -> HealthRow:
        return self._by_name[name]

    def __contains__(self, name) -> bool:
        return name in self._by_name

    def __iter__(self):
        return iter(self.rows)

    def __len__(self):
        return len(self.rows)

    @property
    def first_nonfinite(self) -> Optional[Tuple[str, str]]:
        """("forward" | "backward", name) of the first row, in row order, with a non-finite element -- the forward's first (of the
        last recorded forward) if it has one, else the backward's -- or None."""
        for first in self._first:
            if first >= 0:
                r = self.rows[first]
                return (r.phase, r.name)
        return None

    def worst(self, k: int = 3) -> List[HealthRow]:
        """The k rows of largest absmax (finite elements), largest first; ties in row order."""
        return sorted(self.rows, key=lambda r: -r.absmax)[:max(0, int(k))]

    def fp8_report(self, fmt: str = "e4m3") -> Dict[str, Optional[Dict[str, float]]]:
        """Per row, ``fp8_shares`` of its histogram: the share of finite non-zero elements that stay normal, become subnormal or
        flush under one per-tensor scale that puts absmax at the format's maximum (``fmt``: "e4m3" | "e5m2")."""
        return {r.name: fp8_shares(r.hist, fmt) for r in self.rows}

    def log_line(self) -> str:
        """What fit() writes at log_every: the stage of the first non-finite row, else the three largest absmax rows."""
        bad = self.first_nonfinite
        if bad is not None:
            r = self._by_name[bad[1]]
            return f"health: non-finite first in {bad[0]} row {bad[1]} ({r.nonfinite} of {r.n} elements, {r.nan} NaN)"
        return "health: absmax " + ", ".join(f"{r.name} {r.absmax:.4g}" for r in self.worst(3))
