"""CPU: the drop-in contract.  This package's `FactorizedViViT`, built from the reference's Kinetics-400 config
and given one `TokenNormTopK` per gate the way `utils/misc.py::set_policies` does, must match what the reference's own wrapper
gives on the reference's own `eventful_transformer` -- state_dict keys and shapes (checkpoints load), gate names (set_policies
finds the same gates), policy count and block classes.  The reference's side is stored in tests/golden/dropin_vivit_b.json
(oracle/gen_golden.py::gen_dropin)."""
import json
import os

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_vivit_wrapper_builds_on_this_package(golden_dir):
    import eventful_transformer.blocks as blocks_mod
    from eventful_transformer.policies import TokenNormTopK
    from models.vivit import FactorizedViViT

    with open(os.path.join(golden_dir, "dropin_vivit_b.json")) as f:
        theirs = json.load(f)
    model = FactorizedViViT(**theirs["config"])
    H.set_policies(model, TokenNormTopK, k=theirs["policy_k"])
    gates = [n for n, m in model.named_modules() if type(m).__name__ in ("TokenGate", "TokenDeltaGate")]
    model.reset(); model.counting(); model.clear_counts(); model.no_counting()
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    policies = sum(1 for m in model.modules() if type(m).__name__ == "TokenNormTopK")
    blocks = [type(b).__name__ for b in model.spatial_model.backbone.blocks]
    assert os.path.abspath(blocks_mod.__file__).startswith(ROOT)
    assert keys == theirs["keys"]                    # identical state_dict keys and shapes -> checkpoints load
    assert gates == theirs["gates"]                  # set_policies finds the same gates under the same names
    assert policies == theirs["policies"] == len(gates)
    assert blocks == theirs["blocks"] == ["EventfulBlock"] * 12
