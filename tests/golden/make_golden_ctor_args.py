#!/usr/bin/env python3
"""Mints tests/golden/ctor_args.json: the __init__ argument names of every reference class that the test yaml of tests/test_host_cpu.py
(_YAML) builds with a `!new:cosyvoice.` node, read from the reference sources' AST (the modules themselves need packages that are absent).

    python tests/golden/make_golden_ctor_args.py REFERENCE_TREE

Needs a checkout of the reference; the fixture holds class tags and argument names only.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'ctor_args.json')


def init_args(ref, tag):
    mod, cls = tag.split(':', 1)[1].rsplit('.', 1)
    tree = ast.parse(open(os.path.join(ref, 'server', 'model_utils', *mod.split('.')) + '.py', encoding='utf-8').read())
    c = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    f = next(n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == '__init__')
    return sorted({a.arg for a in f.args.args + f.args.kwonlyargs} - {'self'})


def tags(node, out):
    if isinstance(node, dict):
        if node.get('__tag__', '').startswith('!new:cosyvoice.'):
            out.add(node['__tag__'])
        for v in node.values():
            tags(v, out)
    elif isinstance(node, list):
        for v in node:
            tags(v, out)
    return out


if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    from flowmirror_hydravox_amd.yaml_config import load_hyperpyyaml_plain
    from test_host_cpu import _YAML
    doc = {t: init_args(sys.argv[1], t) for t in sorted(tags(load_hyperpyyaml_plain(_YAML), set()))}
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT, len(doc), 'classes')
