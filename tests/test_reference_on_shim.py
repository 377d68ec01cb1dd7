"""The reference's model package against the MinkowskiEngine shim, from what tests/golden/make_fixtures.py recorded of it
(tests/golden/reference_model_layout.json; the reference's source is not part of this tree):
  * every MinkowskiEngine module its model/*.py import (`import MinkowskiEngine.MinkowskiFunctional as MEF`,
    `from MinkowskiEngine.modules.resnet_block import BasicBlock, Bottleneck`) imports from the shim and has the names
    imported from it, and every ME / MEF attribute the files name exists there (SURVEY 8b "Module import side effects");
  * every ME / MEF call site inside the classes ResUNetBN2C and conv1_max_embedding are made of (constructors and
    forwards), and inside the module-level helpers, binds to the shim's signature: the same number of positional
    arguments and the same keyword names (`MinkowskiNetwork.__init__(self, D)`, `MinkowskiConvolution(in_channels=...,
    dimension=...)`, `SparseTensor(..., coordinate_map_key=..., coordinate_manager=...)`, ...);
  * the project's own reference-named model classes (corsair_amd.model, built on corsair_amd.minkowski, whose classes the
    shim re-exports) have the state-dict names and shapes the reference's models had when built on the shim, which are
    those synth.make_state_dicts produces, and load them.
Runs in a subprocess so the shim's `MinkowskiEngine` never shadows anything in this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "tests", "golden", "reference_model_layout.json")

SCRIPT = r"""
import functools, importlib, inspect, json, sys
import numpy as np
import torch
import MinkowskiEngine as ME
from corsair_amd import synth
from corsair_amd.model import fc, load_model
with open(sys.argv[1]) as f:
    layout = json.load(f)

missing = []
for imp in layout["me_imports"]:
    try:
        mod = importlib.import_module(imp["module"])
    except ImportError as e:
        missing.append("%s (%s: %s)" % (imp["module"], imp["file"], e))
        continue
    missing += ["%s.%s (%s)" % (imp["module"], n, imp["file"]) for n in imp["names"] if not hasattr(mod, n)]
for name in layout["me_names"]:
    try:
        functools.reduce(getattr, name.split("."), ME)
    except AttributeError:
        missing.append(name)
assert not missing, "not on the shim: %r" % missing

built = set(layout["classes_built"])
checked, unbound = 0, []
for c in layout["me_calls"]:
    if not (c["scope"] == "function" or c["where"].split(".")[0] in built):
        continue
    if c["star"]:
        continue                       # *args at the call site: the count is not known statically
    target = functools.reduce(getattr, c["callee"].split("."), ME)
    try:
        inspect.signature(target).bind(*[None] * c["n_args"], **{k: None for k in c["keywords"]})
    except TypeError as e:
        unbound.append("%s:%d %s: %s" % (c["file"], c["line"], c["callee"], e))
    checked += 1
assert not unbound, "call sites the shim's signatures do not accept: %r" % unbound
assert checked >= 30, checked

m = load_model("ResUNetBN2C")(1, 16, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3, D=3)
e = fc.conv1_max_embedding(1024, 512, 256)
sd, emb = synth.make_state_dicts(31)
for mod, want, have in ((m, layout["resunet_bn2c"], sd), (e, layout["conv1_max_embedding"], emb)):
    assert {k: list(v.shape) for k, v in mod.state_dict().items()} == want
    assert {k: list(np.shape(v)) for k, v in have.items()} == want
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in have.items()})
assert len(layout["resunet_bn2c"]) == 129
assert sum(v.numel() for v in m.state_dict().values()) == layout["resunet_bn2c_params"] == 8753669   # SURVEY A.2
print("OK", checked)
"""


def test_reference_model_layout_on_shim(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "shim"), ROOT])
    out = subprocess.run([sys.executable, "-c", SCRIPT, LAYOUT], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-2000:]
