"""The tensors a device-buffer wrapper of hipdev.Context must refuse before its C call, for the *_abi.py tests of those
wrappers (tests/test_pathstep_abi.py, test_compact_abi.py, test_sort_abi.py, test_paths_abi.py)."""
import numpy as np

import torch


def bad_tensors(good, columns):
    """{the refusal's words: a tensor wrong in that one way} for `good`, a CPU tensor (8, columns) right in everything
    else.  A key may end in a blank (two cases, one refusal): strip it."""
    other = columns - 1
    return {"on the GPU": good,  # a CPU tensor, right in everything else
            "must be": good.double() if good.dtype.is_floating_point else good.to(torch.int16),
            "shape": torch.zeros((8, other), dtype=good.dtype),
            "shape ": torch.zeros(8 * columns, dtype=good.dtype),
            "contiguous": torch.zeros((columns, 8), dtype=good.dtype).t(),
            "torch tensor": np.zeros((8, columns), np.float32)}
