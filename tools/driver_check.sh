#!/bin/bash
# GPU box: the end-of-change commands on this tree: smoke(), then the plain N = 1 bench line (exit code, wall seconds, line size,
# the figures) and the --full one (the same, with its roofline, verification and parity objects).
T=$(mktemp -d)
python3 -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
SECONDS=0; python3 bench.py --gpus 1 --steps 20 --warmup 5 > "$T/plain.json" 2> "$T/plain.err"; echo "plain: rc=$? wall ${SECONDS}s"
tail -1 "$T/plain.json" | wc -c
tail -1 "$T/plain.json" | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'])"
SECONDS=0; python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --detail-out "$T/detail.json" > "$T/full.json" 2> "$T/full.err"; echo "full: rc=$? wall ${SECONDS}s"
tail -1 "$T/full.json" | wc -c
tail -1 "$T/full.json" | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline'], d['verified'], d['parity'])"
rm -rf "$T"
