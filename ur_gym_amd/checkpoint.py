"""The checkpoint file of ``SACLearner.save`` / ``SACLearner.load``: ONE ``.npz`` of plain arrays plus one JSON
string, readable with ``allow_pickle=False``.  A state is a tree of dicts and lists whose leaves are numpy arrays or JSON scalars
(int, float, str, bool, None); ``flatten`` moves every array to a flat name (its path, joined with ``/``) and leaves a marker in the
tree, which is then written as JSON under ``META_KEY``; ``unflatten`` is the inverse.  Python's JSON writes a float as its shortest
exact representation and reads ``Infinity`` back, so every scalar survives bit for bit; tuples come back as lists.  Needs no GPU.
"""
import json
import os

import numpy as np

META_KEY = "__checkpoint__"
FORMAT = 1
_ARRAY = "__array__"


def flatten(state):
    """(arrays, tree): `arrays` maps flat names to the numpy arrays of `state`, `tree` is `state` with each array replaced by
    ``{"__array__": name}``.  Raises ValueError for a leaf that is neither an array nor a JSON scalar, and for a key that is not a
    string without ``/``."""
    arrays = {}

    def walk(node, path):
        if isinstance(node, np.ndarray):
            if node.dtype == object:
                raise ValueError(f"checkpoint: {path or '/'} is an object array (the file is read without pickle)")
            arrays[path] = node
            return {_ARRAY: path}
        if isinstance(node, dict):
            out = {}
            for k, v in node.items():
                if not isinstance(k, str) or "/" in k or k in (_ARRAY, ""):
                    raise ValueError(f"checkpoint: the key {k!r} under {path or '/'} must be a non-empty string without '/'")
                out[k] = walk(v, f"{path}/{k}" if path else k)
            return out
        if isinstance(node, (list, tuple)):
            return [walk(v, f"{path}/{i}" if path else str(i)) for i, v in enumerate(node)]
        if isinstance(node, (np.integer, np.bool_)):
            return node.item()
        if isinstance(node, np.floating):
            return float(node)
        if node is None or isinstance(node, (bool, int, float, str)):
            return node
        raise ValueError(f"checkpoint: {path or '/'} holds a {type(node).__name__}; arrays and JSON scalars only")

    tree = walk(state, "")
    if META_KEY in arrays:
        raise ValueError(f"checkpoint: {META_KEY!r} is the name of the JSON string")
    return arrays, tree


def unflatten(arrays, tree):
    """The inverse of ``flatten``: `tree` with every marker replaced by its array."""
    def walk(node):
        if isinstance(node, dict):
            if set(node) == {_ARRAY}:
                if node[_ARRAY] not in arrays:
                    raise ValueError(f"checkpoint: the array {node[_ARRAY]!r} is missing from the file")
                return np.asarray(arrays[node[_ARRAY]])
            return {k: walk(v) for k, v in node.items()}
        if isinstance(node, list):
            return [walk(v) for v in node]
        return node

    return walk(tree)


def write_stream(stream, state):
    """`state` as an uncompressed ``.npz`` into the binary file object `stream` (a file object: numpy appends no suffix of its own)."""
    arrays, tree = flatten(state)
    meta = json.dumps({"format": FORMAT, "state": tree})
    np.savez(stream, **{META_KEY: np.array(meta)}, **{k: np.ascontiguousarray(v) for k, v in arrays.items()})


def temporary_name(path):
    return f"{os.fspath(path)}.tmp"


def write(path, state, opener=open):
    """Writes `state` to ``temporary_name(path)`` through ``opener(name, "wb")``, flushes it to the disk, then renames it onto `path`:
    a writer that dies midway -- a killed job, a full disk -- leaves the previous file at `path` whole, with the unfinished temporary
    file beside it (the next ``write`` starts it again)."""
    tmp = temporary_name(path)
    with opener(tmp, "wb") as f:
        write_stream(f, state)
        f.flush()
        if hasattr(f, "fileno"):
            os.fsync(f.fileno())
    os.replace(tmp, os.fspath(path))


def read(path):
    """The state ``write`` wrote, read with ``allow_pickle=False``.  Raises ValueError for a file that is not such a checkpoint."""
    with np.load(path, allow_pickle=False) as z:
        if META_KEY not in z.files:
            raise ValueError(f"{path}: not a checkpoint (no {META_KEY!r} entry)")
        meta = json.loads(str(z[META_KEY][()]))
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: checkpoint format {meta.get('format')!r}, this library reads {FORMAT}")
        return unflatten({k: z[k] for k in z.files if k != META_KEY}, meta["state"])
