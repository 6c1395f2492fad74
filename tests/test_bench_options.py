"""bench.py's plain run against `--full`: a plain run times the headline and prints its line,
everything measured or checked beside it (oracle check, f32_exact leg, clock probe, captured
variant, CPU baselines, the other configurations) runs only with `--full`."""

import json
import os
import subprocess
import sys

from benchlib import format as fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ('no_check', 'no_exact', 'no_extras', 'no_cpu_baseline', 'no_config3')


def _parse(*argvs):
    'bench.parse_args of each argv, in a process of its own (importing bench sets HSA_* variables).'
    code = ('import json, sys, bench; '
            'print(json.dumps([vars(bench.parse_args(a)) for a in json.loads(sys.argv[1])]))')
    out = subprocess.run([sys.executable, '-c', code, json.dumps(argvs)], cwd=ROOT,
                         check=True, capture_output=True, text=True).stdout
    return json.loads(out.splitlines()[-1])


def test_plain_run_skips_everything_beside_the_headline_and_full_keeps_it():
    plain, plain3, full, full_some = _parse(
        ['--gpus', '1', '--steps', '7', '--warmup', '3'],
        ['--config', '3', '--steps', '2'],
        ['--gpus', '1', '--steps', '7', '--warmup', '3', '--full'],
        ['--full', '--no-cpu-baseline', '--no-config3'])
    for args in (plain, plain3):
        assert not args['full'] and all(args[k] for k in EXTRAS)
    # what the timed steps do is the same either way
    assert (plain['steps'], plain['warmup'], plain['frames']) == (7, 3, 1_000_000)
    assert {k: v for k, v in plain.items() if k != 'full' and k not in EXTRAS} == \
        {k: v for k, v in full.items() if k != 'full' and k not in EXTRAS}
    assert full['full'] and not any(full[k] for k in EXTRAS)
    assert full_some['no_cpu_baseline'] and full_some['no_config3'] and not full_some['no_check']


def test_other_configurations_alone_need_full():
    for flag in ('--config4-only', '--config5-only'):
        res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), flag],
                             cwd=ROOT, capture_output=True, text=True)
        assert res.returncode == 2 and '--full' in res.stderr
    (args,) = _parse(['--config4-only', '--full'])
    assert args['config4_only'] and not args['no_cpu_baseline']


def test_a_plain_line_is_complete():
    'The headline alone -- no parity, cpu_baseline, clock or other configuration -- still formats.'
    out = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench.json')))
    for key in list(out):
        if key.startswith(('config3', 'config4', 'config1', 'config5')) or key in (
                'summary', 'cpu_baseline', 'clock', 'captured', 'f32_exact', 'parity_vs_cpu_fp64',
                'elbo_rel_err_vs_cpu_fp64', 'stats_rel_err_vs_cpu_fp64', 'parity_check'):
            del out[key]
    out['summary'] = fmt.summary(out)
    line = json.loads(fmt.compact_line(out, 'bench_detail.json'))
    for key in fmt.REQUIRED_KEYS:
        assert key in line, key
    assert line['value'] == out['value'] and line['ms_per_step'] == out['ms_per_step']
    assert 'cpu_baseline' not in line and 'parity_vs_cpu_fp64' not in line
    assert set(line['summary']) <= {'config2_frames_per_s', 'config2_ms_per_step',
                                    'config2_roofline_frac'}
