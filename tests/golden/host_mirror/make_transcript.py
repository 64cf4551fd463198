#!/usr/bin/env python3
"""Generates tests/golden/host_mirror/transcript.json: what the host mirror's integrator block hands to the library and
to the backend's set_bcs, recorded by tests/host_mirror_recorder.py without a device and without the library.

Provenance: the fixture is the record of the commit BEFORE a change to that block -- run this on that commit (a worktree
of it with this file, the recorder and tests/test_host_mirror_contract_cpu.py copied in), never on the changed code, and
commit the result with the change.  tests/test_host_mirror_contract_cpu.py then holds the changed code to it.
Re-run:  python tests/golden/host_mirror/make_transcript.py

The file holds every distinct thing once.  `values`: every distinct string of more than 6 characters, list and dict of
the transcript, a list or dict with [n] in the place of each member that is itself value n.  `keys`: the entries' keys
"a|b|c|d" as a tree a -> b -> c -> [n, v, count, v, count, ...]: value n is the list of the tails d, and the entries of
those tails, in that order, are value v (count times), and so on.  `tables`: the boundary-value tables, floats as
float.hex; an entry names one as {"table": index}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import host_mirror_recorder as R  # noqa: E402


def compact(entries, tables):
    values, index = [], {}

    def pack(x):
        if x is None or isinstance(x, (bool, int)) or (isinstance(x, str) and len(x) <= 6):
            return x
        if isinstance(x, list):
            x = [pack(v) for v in x]
        elif isinstance(x, dict):
            x = {k: pack(v) for k, v in x.items()}
        text = json.dumps(x, sort_keys=True)
        if text not in index:
            index[text] = len(values)
            values.append(x)
        return [index[text]]

    keys, tails = {}, {}
    for key, entry in json.loads(json.dumps(entries)).items():
        *head, tail = key.split("|")
        node = keys
        for part in head[:-1]:
            node = node.setdefault(part, {})
        runs = node.setdefault(head[-1], [])
        tails.setdefault(id(runs), (runs, []))[1].append(tail)
        v = pack(entry)[0]
        if runs and runs[-2] == v:
            runs[-1] += 1
        else:
            runs += [v, 1]
    for runs, t in tails.values():
        runs.insert(0, pack(t)[0])
    return {"tables": tables, "values": values, "keys": keys}


def expand(fixture):
    """(entries by key, tables) of a fixture"""
    values = fixture["values"]

    def unpack(x):
        if isinstance(x, list):
            x = values[x[0]]
            if isinstance(x, list):
                return [unpack(v) for v in x]
            if isinstance(x, dict):
                return {k: unpack(v) for k, v in x.items()}
        return x

    out = {}

    def walk(head, node):
        if isinstance(node, dict):
            for part, child in node.items():
                walk(head + part + "|", child)
            return
        tails = iter(unpack([node[0]]))
        for v, count in zip(node[1::2], node[2::2]):
            for _ in range(count):
                out[head + next(tails)] = unpack([v])

    walk("", fixture["keys"])
    return out, fixture["tables"]


if __name__ == "__main__":
    entries, tables = R.transcript()
    fixture = compact(entries, tables)
    assert expand(fixture)[0] == json.loads(json.dumps(entries))
    path = os.path.join(HERE, "transcript.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(fixture, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{len(entries)} entries, {len(fixture['values'])} distinct values, {len(tables)} tables, "
          f"{os.path.getsize(path)} bytes -> {path}")
