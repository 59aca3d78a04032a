"""What the analyses over many segments or clips share on the host side: stacking the maps of a job, the leading arguments
of the two standard sources (maps the caller holds, PCM clips behind the model), the sample rates of a job and the loops over
its rate groups, the decodes of a sweep, and the record arrays the score calls bring home.  `events`, `sweep`, `score`,
`frame_score`, `multipitch`, `melody`, `align`, `beat`, `chord` and `sync` call into it; a new analysis starts from it and adds its
parameters, its result class and its one native-call wrapper.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from . import note_creation as _notes

_pi64 = C.POINTER(C.c_int64)

Pair = Tuple[int, int]  # (segment, set)


def offsets_of(rows: Sequence[int]) -> np.ndarray:
    """Counts per segment -> offsets as int64 [n + 1]: offsets[i] = the count before segment i, offsets[-1] = all."""
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def stack(outputs: Sequence[Any], planes: Sequence[str], what: str, bare: bool = False, mismatch: Optional[str] = None):
    """The `planes` (of note, onset, contour) of posteriorgram dicts (numpy arrays or CUDA tensors, all of one kind; `bare`: a
    map alone is taken in place of a dict) as the maps calls take them: (row offsets, {plane: the maps of all segments one after
    the other}, {plane: pointer, or None without rows}, mem_kind).  The pointers are into the returned maps, which the caller
    holds until its call has returned.  `mismatch`: the caller's own words for planes that disagree in rows or memory kind."""
    from . import inference as _inf

    maps, kinds, rows = {}, [], []
    for k, w in _inf._MAPS:
        if k not in planes:
            continue
        on_dev, parts = None, []
        for out in outputs:
            a = out if bare and not isinstance(out, dict) else out[k]
            on_dev = _inf._is_torch_cuda(a) if on_dev is None else on_dev
            if _inf._is_torch_cuda(a) != on_dev:
                raise ValueError(f"{what}: the maps must all be numpy arrays or all CUDA tensors")
            a = a.contiguous().float() if on_dev else np.require(a, np.float32, ["C"])
            if a.ndim != 2 or a.shape[1] != w:
                raise ValueError(f"{k}: expected (T, {w})")
            parts.append(a)
        if on_dev:
            import torch

            maps[k] = torch.cat(parts) if len(parts) > 1 else parts[0]
        else:
            maps[k] = np.concatenate(parts) if len(parts) > 1 else parts[0]
        kinds.append(on_dev)
        rows.append([int(a.shape[0]) for a in parts])
    if any(kind != kinds[0] for kind in kinds):
        raise ValueError(mismatch or f"{what}: the maps must all be numpy arrays or all CUDA tensors")
    if any(r != rows[0] for r in rows):
        raise ValueError(mismatch or f"{what}: note, onset and contour of a segment must have the same number of rows")
    offs = offsets_of(rows[0])
    first = next(iter(maps.values()))
    if kinds[0]:
        import torch

        torch.cuda.current_stream(first.device).synchronize()
    ptrs = {k: (_inf._ptr(a) if int(offs[-1]) else None) for k, a in maps.items()}
    return offs, maps, ptrs, _inf._mem_kind(first)


def maps_source(model: Any, row_offsets: Sequence[int], ptrs: Sequence[Any], mem_kind: int) -> Tuple[tuple, np.ndarray]:
    """The leading arguments of a given-maps call, `handle, n, row_offsets, <plane pointers>, mem_kind`, and the offsets as the
    int64 array the tuple points into (the pointer object holds it)."""
    offs = np.ascontiguousarray(row_offsets, np.int64)
    return (model._handle, len(offs) - 1, offs.ctypes.data_as(_pi64), *ptrs, int(mem_kind)), offs


def clips_source(model: Any, arrays: Sequence[np.ndarray], sample_rate: int) -> tuple:
    """The leading arguments of a PCM-clips call, `handle, n, clip_table, sample_rate, BP_MEM_HOST`; the tuple holds the table,
    the caller the arrays behind it."""
    from . import clips as _clips

    return (model._handle, len(arrays), _clips.clip_table(arrays), int(sample_rate), _native.BP_MEM_HOST)


def rates_of(arrays: Sequence[Any], sample_rates: Union[int, Sequence[int]]) -> List[int]:
    """`sample_rates`, one int for all or one per clip, as one int per clip."""
    if isinstance(sample_rates, (int, np.integer)):
        return [int(sample_rates)] * len(arrays)
    rates = [int(r) for r in sample_rates]
    if len(rates) != len(arrays):
        raise ValueError(f"{len(arrays)} clips but {len(rates)} sample rates")
    return rates


def rate_groups(rates: Sequence[int]) -> List[Tuple[int, List[int]]]:
    """[(rate, the indices of its clips)], the rates by first appearance."""
    return [(rate, [i for i, r in enumerate(rates) if r == rate]) for rate in dict.fromkeys(rates)]


def per_rate(rates: Sequence[int], run: Callable[[List[int], int], Sequence[Any]]) -> List[Any]:
    """One `run(ids, rate)` per rate group, which returns one result per clip of the group: the results in input order."""
    results: List[Any] = [None] * len(rates)
    for rate, ids in rate_groups(rates):
        for i, res in zip(ids, run(ids, rate)):
            results[i] = res
    return results


def per_rate_swept(todo: Sequence[Pair], rates: Sequence[int], run: Callable[[List[int], int, List[Pair]], Any]
                   ) -> Iterator[Tuple[int, int, int, Any]]:
    """One `run(ids, rate, local_pairs)` per rate that a pair of `todo` names; local_pairs are the group's pairs in `todo`
    order, the segment renumbered to its index within the group.  Yields per decode (j, k, rate, reply): its position in
    `todo`, its index in the group's reply, and that reply; a group's decodes come before the next group's call."""
    for rate, ids in rate_groups(rates):
        local = {i: k for k, i in enumerate(ids)}
        mine = [j for j, (s, _) in enumerate(todo) if s in local]
        if not mine:
            continue
        reply = run(ids, rate, [(local[todo[j][0]], todo[j][1]) for j in mine])
        for k, j in enumerate(mine):
            yield j, k, rate, reply


def cross_product(n_sets: int, n_segments: int) -> List[Pair]:
    """The decodes a call without a table runs, in its order: set-major, decode p * n_segments + i is (segment i, set p)."""
    return [(i, p) for p in range(n_sets) for i in range(n_segments)]


def pairs_checked(pairs: Optional[Sequence[Pair]], n_seg: int, n_sets: int, what: str, refs: Optional[Sequence[Any]] = None
                  ) -> List[Pair]:
    """The decodes of a sweep as a list, `pairs` None being the cross product; ValueError for a pair out of range, and for
    `refs` (where the call has them) that are not one per segment."""
    if refs is not None and len(refs) != n_seg:
        raise ValueError(f"{what}: {n_seg} segments but refs for {len(refs)}")
    todo = list(pairs) if pairs is not None else cross_product(n_sets, n_seg)
    if any(not (0 <= s < n_seg and 0 <= p < n_sets) for s, p in todo):
        raise ValueError(f"{what}: a pair names a segment outside 0..{n_seg - 1} or a set outside 0..{n_sets - 1}")
    return todo


def decode_table(pairs: Sequence[Pair]):
    """The `bp_sweep_decode` array of (segment, set) pairs."""
    tab = (_native.bp_sweep_decode * max(1, len(pairs)))()
    for j, (seg, p) in enumerate(pairs):
        tab[j] = _native.bp_sweep_decode(int(seg), int(p), 0)
    return tab


def decodes_block(sets: Any, n_sets: int, pairs: Optional[Sequence[Pair]], n_segments: int) -> Tuple[tuple, int]:
    """The arguments `n_sets, sets, n_decodes, decodes` of a sweep call, and n_decodes.  `sets`: the caller's ctypes array, which
    it holds; the decode table (None without `pairs`: the cross product) goes into the tuple as the array itself."""
    n = len(pairs) if pairs is not None else n_sets * n_segments
    return (n_sets, C.addressof(sets), n, decode_table(pairs) if pairs is not None else None), n


def records(dtype: np.dtype, table: np.ndarray, status: np.ndarray, n: int) -> np.ndarray:
    """`n` records of `dtype`: field i from column i of the integer `table`, the last field, status, from `status`."""
    out = np.zeros(n, dtype)
    for i, name in enumerate(dtype.names[:-1]):
        out[name] = table[:n, i]
    out["status"] = status[:n]
    return out


def host_decode(maps: Sequence[np.ndarray], prm: Any) -> List["_notes.NoteEvent"]:
    """The host decoder (`bp_notes_decode`) on the float32 note, onset and contour maps of one segment; it may write to the
    first two, so the caller hands it copies."""
    T = int(maps[0].shape[0])
    decoded = _notes._grow_and_call(_native.load_library().bp_notes_decode, tuple(m.ctypes.data for m in maps) + (T, C.byref(prm)),
                                    T, "bp_notes_decode")
    return _notes._note_events(*decoded, bool(prm.include_pitch_bends))
