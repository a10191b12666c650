#!/bin/bash
# Run on an MI355X from the repo root: tools/final_measure.sh [output dir, default bench_out] -- the round's closing
# measurements (GPU test suite, every bench configuration with --full), results under <output dir>/r3_final_*.json, one
# summary line each.
out=${1:-bench_out}
mkdir -p "$out"
python -m pytest tests -m gpu -x -q 2>&1 | tail -1
A=config/ar_vae_dente_kl1e3.json; R=config/reg_edente_from_dente.json
python bench.py --full --steps 30 --warmup 8 --detail-out "$out/r3_final_A_per_shape.json" > "$out/r3_final_A.json" 2>/dev/null
python bench.py --full --steps 30 --warmup 8 --no-cpu-baseline --channels 3 > "$out/r3_final_A3.json" 2>/dev/null
for b in 8 32; do
  python bench.py --full --steps 15 --warmup 4 --no-cpu-baseline --config $A --batch $b > "$out/r3_final_AR$b.json" 2>/dev/null
  python bench.py --full --steps 30 --warmup 8 --no-cpu-baseline --config $R --batch $b > "$out/r3_final_reg$b.json" 2>/dev/null
done
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --adv > "$out/r3_final_A_adv.json" 2>/dev/null
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --perceptual > "$out/r3_final_A_perc.json" 2>/dev/null
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --adv --perceptual > "$out/r3_final_A_full.json" 2>/dev/null
python bench.py --full --steps 15 --warmup 4 --no-cpu-baseline --adv --config $A --batch 8 > "$out/r3_final_AR8_adv.json" 2>/dev/null
python bench.py --full --steps 15 --warmup 4 --no-cpu-baseline --adv --perceptual --config $A --batch 8 > "$out/r3_final_AR8_full.json" 2>/dev/null
for f in A A3 AR8 AR32 reg8 reg32 A_adv A_perc A_full AR8_adv AR8_full; do
  python -c "
import json
d=json.loads(open('$out/r3_final_$f.json').read().strip().splitlines()[-1]); print('$f', d['ms_per_step'], d['value'], d.get('model_tflops_per_gpu'))"
done
