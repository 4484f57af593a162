"""Generate tests/golden/reference_modules.npz from the REAL reference's field and encoding modules (model.py, embedding.py) on CPU.

Run where the reference source tree exists (VMAP_REFERENCE_ROOT, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_module_goldens.py

Per hidden width (32, 128): the parameter names in ``named_parameters()`` order, the state dict of a freshly initialised
``model.OccupancyMap`` (``torch.manual_seed(H)``, ``init_weights``), a random embedding and the module's two outputs on it.  Per
encoding scale (2.0, 5.0): the state-dict keys, parameter and buffer names of ``embedding.UniDirsEmbed``, its buffers and
``B_layer.weight`` as built, then - with 0.01 added to ``B_layer.weight`` - its state dict, a random input and the output on it.
``tests/test_host_logic.py::test_state_dicts_interchange_with_the_reference_modules_both_ways`` checks ``vmap_amd.fields`` against it.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VMAP_REFERENCE_ROOT", "/root/reference")


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    model, embedding = importlib.import_module("model"), importlib.import_module("embedding")
    out = {"torch_version": np.array(torch.__version__)}
    for H in (32, 128):
        torch.manual_seed(H)
        m = model.OccupancyMap(87, 42, hidden_size=H)
        m.apply(model.init_weights)
        emb = torch.randn(7, 5, 129)
        with torch.no_grad():
            alpha, color = m(emb)
        out[f"H{H}_param_names"] = np.array([n for n, _ in m.named_parameters()])
        out[f"H{H}_state_keys"] = np.array(list(m.state_dict()))
        for k, v in m.state_dict().items():
            out[f"H{H}_state.{k}"] = v.numpy()
        out[f"H{H}_emb"], out[f"H{H}_alpha"], out[f"H{H}_color"] = emb.numpy(), alpha.numpy(), color.numpy()
    for scale in (2.0, 5.0):
        pe = embedding.UniDirsEmbed(max_deg=5, scale=scale)
        p = f"pe{scale:g}"
        out[f"{p}_state_keys"] = np.array(list(pe.state_dict()))
        out[f"{p}_param_names"] = np.array([n for n, _ in pe.named_parameters()])
        out[f"{p}_buffer_names"] = np.array([n for n, _ in pe.named_buffers()])
        out[f"{p}_B_layer_weight"] = pe.B_layer.weight.detach().numpy().copy()
        out[f"{p}_frequency_bands"], out[f"{p}_scale"] = pe.frequency_bands.numpy(), pe.scale.numpy()
        with torch.no_grad():
            pe.B_layer.weight.add_(0.01)
        for k, v in pe.state_dict().items():
            out[f"{p}_state.{k}"] = v.numpy()
        torch.manual_seed(int(scale))
        x = torch.randn(11, 3)
        with torch.no_grad():
            out[f"{p}_x"], out[f"{p}_out"] = x.numpy(), pe(x).numpy()
    np.savez_compressed(os.path.join(HERE, "reference_modules.npz"), **out)


if __name__ == "__main__":
    main()
