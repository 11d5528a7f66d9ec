#!/bin/bash
# usage (GPU box, repo root): tools/ab_files.sh "<file.hip> ..." "<grep over [kernel] lines>" [bench args]
# A/B on ONE box: the tree as it is ("new") against the same tree with the listed csrc files replaced by their copies under
# tools/build/old/ ("old"), alternating new, old, new2, old2 so that each side's own spread is on the page; each variant is built in
# a scratch copy and benched; prints what was compiled, the library's checksum, fps and the matching [kernel] lines.  A build or a bench that fails ends the run.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
files=$1; pat=${2:-.}; shift; shift
for v in new old new2 old2; do
  rm -rf /tmp/ab_$v && mkdir -p /tmp/ab_$v && cp -r hdr-realtime-video-pipeline_amd include tools tests bench.py oracle /tmp/ab_$v/; [ -f BASELINE.json ] && cp BASELINE.json /tmp/ab_$v/
  if [ ${v%2} = old ]; then for f in $files; do cp tools/build/old/$f /tmp/ab_$v/hdr-realtime-video-pipeline_amd/csrc/$f || exit 1; done; touch /tmp/ab_$v/hdr-realtime-video-pipeline_amd/csrc/*.hip; fi
  (cd /tmp/ab_$v/hdr-realtime-video-pipeline_amd/csrc && for f in $files; do touch $f; done && make -j8 > /tmp/ab_$v.make 2>&1) || { grep -E "error" /tmp/ab_$v.make; echo "$v: build failed"; exit 1; }
  echo "$v built: $(grep -c -- ' -c ' /tmp/ab_$v.make) files compiled, library sha1 $(sha1sum < /tmp/ab_$v/hdr-realtime-video-pipeline_amd/lib/libhdrtv_mi355x.so | cut -c1-12)"
  (cd /tmp/ab_$v && timeout -k 10 420 python bench.py --full --steps 20 --warmup 5 --layers --no-cpu-baseline --no-int8-extra --no-dispatcher "$@" 2> /tmp/ab_$v.err | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['value'], d['p50_ms'])") || { tail -5 /tmp/ab_$v.err; echo "$v: bench failed"; exit 1; }
  grep "^\[kernel\]" /tmp/ab_$v.err | grep -E "$pat" | cut -c1-110
done
