"""The oracle's stub-import of the reference must not leak its ``lightning`` test double into the product package
(a reference import followed by tests/test_checkpoint_keys.py failed in that order).

The reference sources are replaced by a stand-in tree of the same layout whose ``models/lightning.py`` binds
``lightning.LightningModule`` at class creation, as the reference's does: that binding is what made the stub leak."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STAND_IN = {
    "models/__init__.py": "",
    "models/nunet.py": "import torch.nn as nn\n\n\nclass TowerUNet(nn.Module):\n    pass\n",
    "models/lightning.py": "from lightning import LightningModule\n\n\nclass CultionetLitModel(LightningModule):\n    pass\n",
    "losses/__init__.py": "",
}


def test_reference_import_then_product_import_in_a_fresh_interpreter(tmp_path):
    src = tmp_path / "cultionet"
    for rel, text in STAND_IN.items():
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        (src / rel).write_text(text)
    code = (
        "import sys\n"
        "from oracle import refimport\n"
        f"refimport.REF_SRC = {str(src)!r}\n"
        "ns = refimport.import_reference()\n"
        "assert ns.CultionetLitModel.__mro__[1].__qualname__.startswith('import_reference.'), 'not the lightning stub'\n"
        "assert not getattr(sys.modules.get('lightning'), '_oracle_stub', False), 'stub lightning left in sys.modules'\n"
        "import cultionet_amd.lightning as L\n"
        "assert hasattr(L.CultionetLitModel, 'load_from_checkpoint')\n"
        "assert ns.CultionetLitModel is not L.CultionetLitModel\n"
    )
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
