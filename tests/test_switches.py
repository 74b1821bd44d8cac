"""CPU: every environment switch the engine reads is under test or named exempt below, and DESIGN.md 8 lists exactly the
switches that are read."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sixty-years-of-frequency-domain-monaural-speech-enhancement_amd')

# measurement and tool switches: no test sets them
EXEMPT = {
    'SE_GRAPH': 'tools/sweep.py replays decodes from hipGraphs with it',
    'SE_GRAPH_FORK': 'the one-stream valve for replayed decodes of the forking models',
    'SE_PROF_DUMP': 'per-launch lines for tools/profl.py',
    'SE_COOP_DBG': 'cooperative LSTM ablations (csrc/tools/coopbench.cpp, profiles/)',
    'SE_TCM_DBG': 'fused TCM kernel ablations (profiles/)',
    'SE_ENGINE_LIB': 'loads another build of the library for A/B runs of two builds',
}

READ = re.compile(r'''getenv\("(SE_[A-Z0-9_]+)"|os\.environ(?:\.get\(|\[)\s*['"](SE_[A-Z0-9_]+)''')


def switches_read():
    files = glob.glob(os.path.join(PKG, 'csrc', '*.hip')) + glob.glob(os.path.join(PKG, 'csrc', '*.h')) + \
        glob.glob(os.path.join(PKG, '*.py'))
    return {a or b for f in files for a, b in READ.findall(open(f).read())}


def design_listed():
    """the variables named in the first column of the table rows of DESIGN.md 8 (the second column also names se_config flags)"""
    sec = re.search(r'\n## 8\..*?(?=\n## |\Z)', open(os.path.join(ROOT, 'DESIGN.md')).read(), re.S).group(0)
    return {s for row in sec.splitlines() if row.startswith('| `') for s in re.findall(r'SE_[A-Z0-9_]+', row.split('|')[1])}


def test_every_switch_is_tested_or_exempt():
    tests = ''.join(open(f).read() for f in glob.glob(os.path.join(ROOT, 'tests', '*.py'))
                    if os.path.basename(f) != os.path.basename(__file__))
    untested = {s for s in switches_read() if s not in EXEMPT and not re.search(r'\b%s\b' % s, tests)}
    assert not untested, sorted(untested)


def test_every_switch_has_a_design_row():
    assert not switches_read() - design_listed(), sorted(switches_read() - design_listed())


def test_every_design_row_names_a_switch_that_is_read():
    assert not design_listed() - switches_read(), sorted(design_listed() - switches_read())
