"""The case names that tests/test_gpu_*.py hand to routecheck.run_case exist in the child module they name, and every case of a child
module is run by some test: read from the sources with ast, so a mistyped or orphaned name is found without a GPU (and without torch)."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def parse(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def cases_run():
    """{child module: {case names}} over every run_case(module, case, ...) call of tests/test_gpu_*.py; `case` is a literal, or the
    parameter of a test whose parametrize list holds the literals"""
    run = {}
    for path in sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py"))):
        for fn in [n for n in ast.walk(parse(path)) if isinstance(n, ast.FunctionDef)]:
            calls = [n for n in ast.walk(fn) if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "run_case"]
            listed = {}
            for deco in fn.decorator_list if calls else []:
                if isinstance(deco, ast.Call) and getattr(deco.func, "attr", "") == "parametrize":
                    listed[ast.literal_eval(deco.args[0])] = ast.literal_eval(deco.args[1])
            for call in calls:
                module, case = ast.literal_eval(call.args[0]), call.args[1]
                run.setdefault(module, set()).update([case.value] if isinstance(case, ast.Constant) else listed[case.id])
    return run


def functions_of(module):
    return [n for n in parse(os.path.join(HERE, module + ".py")).body if isinstance(n, ast.FunctionDef)]


def test_every_case_that_is_run_exists():
    run = cases_run()
    assert len(run) >= 11 and sum(len(v) for v in run.values()) >= 47
    for module, names in run.items():
        have = {f.name for f in functions_of(module)}
        assert names <= have, (module, sorted(names - have))


def test_every_case_of_a_child_module_is_run():
    run = cases_run()
    modules = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(HERE, "*_torch_cases.py")))
    assert len(modules) == 10 and set(modules) <= set(run)
    for module in modules:
        fns = functions_of(module)
        called = {n.func.id for f in fns for n in ast.walk(f) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}      # helpers of other cases
        cases = {f.name for f in fns if f.args.args and f.args.args[0].arg == "rt"}
        assert cases - called <= run[module], (module, sorted(cases - called - run[module]))
