set -o pipefail
out=${1:?usage: tools/final_check.sh OUTDIR}
mkdir -p $out
python -m pytest tests -m gpu -x -q > $out/pytest.log 2>&1; rc=$?; tail -n 3 $out/pytest.log; [ $rc -eq 0 ] || exit $rc
python bench.py --full > $out/bench.json 2> $out/bench.err || exit 1
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print('bf16', d['value'], d['ms_per_step'], d['roofline']['frac'], d['power']); a=d['also']['configs4_fp8_per_gpu']; print('fp8', a['value'], a['ms_per_step'], a['roofline']['frac'], a['power']); print('bucketed', d['also']['configs3_bucketed']['value']); print({k:v for k,v in d['config'].items() if 'logit' in k or 'latent' in k or 'within' in k})" $out/bench.json
timeout -k 10 400 python tools/soak.py 200 16 11=1 > $out/soak_fp8.log 2>&1; tail -n 2 $out/soak_fp8.log
timeout -k 10 400 python tools/soak.py 100 16 > $out/soak_bf16.log 2>&1; tail -n 2 $out/soak_bf16.log
