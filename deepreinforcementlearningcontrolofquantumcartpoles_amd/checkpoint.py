"""Checkpoint and bit-exact resume of a device training loop.

Every stateful object of the loop exports what its next call reads (`state_dict()` on Stepper, MeasurementRecord,
BatchedEnv, DQNActor, MeasurementActor and PrioritizedReplay; `train_state()` on the two learners, whose
`state_dict()` is the weights in the reference's keys) and takes it back (`load_state_dict()` /
`load_train_state()`). Every component is deterministic, so a run continued from a checkpoint is the same run,
bit for bit, as one that was never stopped (tests/test_gpu_checkpoint.py).

    objects = {"env": env, "actor": actor, "memory": memory, "learner": learner}
    checkpoint.save(path, objects, extra={"calls": calls})          # any time between two calls of the loop
    ...
    # a new process: build the same objects with the same arguments (any initial weights), then
    extra = checkpoint.load(path, objects)

A state is a plain dict of CPU tensors, ints, floats, strings, lists and tuples, so the file loads with
`torch.load(weights_only=True)`. Both functions synchronise the device: save copies every buffer to the host (the
replay memory as one piece: capacity * (row_len * 4 + 16) bytes once the ring is full), load copies them back.
Nothing is converted: an object made for another batch, capacity, net, input, reset mode, env_offset or seed is
refused with an error that names the field, before any object is changed.
"""
from __future__ import annotations

import os
import tempfile
from typing import Any, Mapping, Optional

import torch

FORMAT = 1


def _methods(obj):
    """(export, check or None, import) of an object: the learners' train_state trio, else the state_dict one."""
    if hasattr(obj, "train_state"):
        return obj.train_state, getattr(obj, "check_train_state", None), obj.load_train_state
    return obj.state_dict, getattr(obj, "check_state_dict", None), obj.load_state_dict


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def save(path, objects: Mapping[str, Any], extra: Optional[Any] = None) -> None:
    """Write {"format": 1, "objects": {name: state}, "extra": extra} to `path`: with torch.save to a temporary
    file in the same directory, then os.replace, so a failure leaves an existing file intact. `extra` must be made
    of what weights_only loading admits (tensors, numbers, strings, lists, tuples, dicts). Synchronises the device."""
    _sync()
    doc = {"format": FORMAT, "objects": {name: _methods(obj)[0]() for name, obj in objects.items()}, "extra": extra}
    path = os.fspath(path)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path) or ".")
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(doc, f)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def load(path, objects: Mapping[str, Any]) -> Any:
    """Read a file `save` wrote into `objects` (the same names) and return its `extra`. The file is read with
    torch.load(map_location="cpu", weights_only=True). Every named object must be in the file and must accept its
    state's echo (check_state_dict / check_train_state); only then is the first object changed. A ValueError names
    what is missing or differs. Synchronises the device."""
    doc = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(doc, dict) or doc.get("format") != FORMAT:
        fmt = doc.get("format") if isinstance(doc, dict) else type(doc).__name__
        raise ValueError(f"checkpoint: unknown format {fmt!r} (this version reads format {FORMAT})")
    states = doc.get("objects")
    if not isinstance(states, dict):
        raise ValueError("checkpoint: the file has no 'objects' dict")
    missing = [name for name in objects if name not in states]
    if missing:
        raise ValueError(f"checkpoint: the file has no object named {missing[0]!r} (it has {sorted(states)})")
    for name, obj in objects.items():
        check = _methods(obj)[1]
        if check is not None:
            try:
                check(states[name])
            except ValueError as e:
                raise ValueError(f"checkpoint: object {name!r}: {e}") from e
    _sync()
    for name, obj in objects.items():
        _methods(obj)[2](states[name])
    _sync()
    return doc.get("extra")


__all__ = ["save", "load", "FORMAT"]
