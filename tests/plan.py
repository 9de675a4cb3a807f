"""Recording the plan (no tests here): the engine's specs on the meta device and a dispatch mode that writes down every op that
reaches the dispatcher — tests/test_plan_cpu.py pins the rows against its fixture, tests/test_custom_ops_cpu.py walks the registered
ops with them."""
import dataclasses
import functools

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves

import hilcodec_amd
from hilcodec_amd import engine, synth


@functools.lru_cache(maxsize=None)
def specs(model_name, streaming):
    mk = dict(synth.model_kwargs(model_name))
    sd = synth.synth_state_dict(model_name, seed=7)
    if streaming:
        m = synth.streaming_model(model_name, state_dict=sd)
    else:
        m = hilcodec_amd.HILCodec(24000, 1, **mk).eval()
        m.load_state_dict(sd, strict=False)
    return tuple(engine.finalize_spec(engine.spec_to(half.build_spec("cpu"), "meta"), streaming=streaming) for half in (m.encoder, m.decoder))


class Recorder(TorchDispatchMode):
    """rows = [op name, [arguments], {keyword arguments}] of every op that reaches the dispatcher, ATen ones included; a tensor is
    written as its name, and the outputs of op k are named `#k.j`"""

    def __init__(self):
        super().__init__()
        self.names = {}         # id(tensor) -> name
        self.keep = []          # ... and the tensors themselves: an id must not be handed out twice
        self.rows = []

    def name(self, t, name):
        if id(t) not in self.names:
            self.names[id(t)] = name
            self.keep.append(t)

    def name_tree(self, obj, path):
        if isinstance(obj, torch.Tensor):
            self.name(obj, path)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                self.name_tree(v, f"{path}[{i}]")
        elif dataclasses.is_dataclass(obj):
            for f in dataclasses.fields(obj):
                self.name_tree(getattr(obj, f.name), f"{path}.{f.name}")

    def _enc(self, a, where):
        if isinstance(a, torch.Tensor):
            assert id(a) in self.names, f"{where}: a tensor {tuple(a.shape)} that is neither a spec field, an input, a cache nor an op's output"
            return self.names[id(a)]
        if isinstance(a, (list, tuple)):
            return [self._enc(v, where) for v in a]
        return repr(a)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        k = len(self.rows)
        op = func._schema.name.replace("::", ".") + ("." + func._overloadname if func._overloadname else "")
        where = f"op {k} {op}"
        self.rows.append([op, [self._enc(a, where) for a in args], {n: self._enc(v, where) for n, v in sorted(kwargs.items())}])
        out = func(*args, **kwargs)
        for j, t in enumerate(tree_leaves(out)):
            if isinstance(t, torch.Tensor):
                self.name(t, f"#{k}.{j}")
        return out


def launches(rows):
    return [r[0][len("hilcodec."):] for r in rows if r[0].startswith("hilcodec.")]
