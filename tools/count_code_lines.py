"""Code lines of multidevice.py + plugins/*.py: no blank, comment or docstring lines (ast + tokenize).

    python tools/count_code_lines.py [repository root]
"""
import ast, glob, io, sys, tokenize
def code_lines(path):
    src = open(path).read()
    drop = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            d = node.body[0]
            if isinstance(d, ast.Expr) and isinstance(d.value, ast.Constant) and isinstance(d.value.value, str):
                drop.update(range(d.lineno, d.end_lineno + 1))
    keep = set()
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type not in (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER):
            keep.update(range(tok.start[0], tok.end[0] + 1))
    return len(keep - drop)
root = sys.argv[1] if len(sys.argv) > 1 else "."
files = [root + "/waveformanalysis_amd/multidevice.py"] + sorted(glob.glob(root + "/waveformanalysis_amd/plugins/*.py"))
print(sum(code_lines(f) for f in files))
