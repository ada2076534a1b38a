#!/usr/bin/env python3
"""Record what tests/test_cpu_import_surface.py checks the drop-in against, from a checkout of the reference:

    python tools/dump_reference_surface.py --reference /path/to/InconsistencyMasks

writes tests/golden/reference_surface.json with
  * scripts       every reference script under ISIC_2018/ HeLa/ SUIM/ Cityscapes/ that has a counterpart here,
  * wanted        every name those scripts take from `functions`, `unet`, `evalnet`, `paths`, the class-mapping modules and the
                  TensorFlow namespace ("from:<module>:<name>" and "chain:<module>:<dotted attribute>"), each with the scripts that
                  use it -- read from the scripts' syntax trees,
  * class_tables  every upper-case name of the reference's SUIM/SUIM_class_mapping.py and Cityscapes/Cityscapes_class_mapping.py,
                  as the repr of its value (colour tuples -> class ids, class descriptions).
Only names and table values are written: no reference source text.  The test then needs nothing outside this repository."""
import argparse
import ast
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_surface.json")
DATASETS = ("ISIC_2018", "HeLa", "SUIM", "Cityscapes")
SHIMMED = {"functions", "unet", "evalnet", "paths", "SUIM_class_mapping", "Cityscapes_class_mapping"}
TABLES = (("SUIM", "SUIM_class_mapping"), ("Cityscapes", "Cityscapes_class_mapping"))


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
        return ".".join(reversed(parts))
    return None


def surface(path):
    """-> (from-imports {module: {names}}, attribute chains rooted at an imported module alias {alias: {dotted}}, alias -> module)"""
    tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
    froms, alias = {}, {}
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and n.module:
            froms.setdefault(n.module, set()).update(a.name for a in n.names)
            for a in n.names:
                alias[a.asname or a.name] = f"{n.module}.{a.name}"
        elif isinstance(n, ast.Import):
            for a in n.names:
                alias[a.asname or a.name.split(".")[0]] = a.name if a.asname else a.name.split(".")[0]
    chains = {}
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute):
            d = _dotted(n)
            if d and d.split(".")[0] in alias:
                chains.setdefault(d.split(".")[0], set()).add(d)
    return froms, chains, alias


def scripts(ref):
    out = []
    for ds in DATASETS:
        for f in sorted(os.listdir(os.path.join(ROOT, ds))):
            if f.endswith(".py") and os.path.exists(os.path.join(ref, ds, f)):
                out.append(f"{ds}/{f}")
    return out


def wanted_names(ref, paths):
    wanted = {}     # "from:module:name" or "chain:<module>:<dotted>" -> scripts that need it
    for p in paths:
        froms, chains, alias = surface(os.path.join(ref, p))
        for mod, names in froms.items():
            top = mod.split(".")[0]
            if top in SHIMMED or top in ("tensorflow", "tensorflow_addons"):
                for n in names:
                    wanted.setdefault(f"from:{mod}:{n}", []).append(p)
        for a, ds_ in chains.items():
            target = alias[a].split(".")[0]
            if target in SHIMMED or target in ("tensorflow", "tensorflow_addons"):
                # keep the longest chains only (tf.keras.models.load_model implies tf.keras.models)
                longest = {d for d in ds_ if not any(o != d and o.startswith(d + ".") for o in ds_)}
                for d in longest:
                    wanted.setdefault(f"chain:{alias[a]}:{d.split('.', 1)[1]}", []).append(p)
    return {k: sorted(set(v)) for k, v in sorted(wanted.items())}


def class_tables(ref):
    out = {}
    for ds, mod in TABLES:
        spec = importlib.util.spec_from_file_location("ref_" + mod, os.path.join(ref, ds, mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        out[mod] = {n: repr(v) for n, v in sorted(vars(m).items()) if n.isupper()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    paths = scripts(a.reference)
    rec = {"scripts": paths, "wanted": wanted_names(a.reference, paths), "class_tables": class_tables(a.reference)}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {len(paths)} scripts, {len(rec['wanted'])} names, {sum(map(len, rec['class_tables'].values()))} tables")


if __name__ == "__main__":
    main()
