"""One `.npz` without pickled objects (`np.load(path, allow_pickle=False)` reads it): arrays by name and `meta`, a dict, as a JSON string."""
import json

import numpy as np


def save(path, meta, **arrays):
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    return path


def load(path, *names):      # -> (the arrays `names` ..., meta) of a file written by `save`
    with np.load(path, allow_pickle=False) as f:
        return (*(f[k] for k in names), json.loads(str(f["meta"][()])))
