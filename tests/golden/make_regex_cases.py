#!/usr/bin/env python3
"""Reads the (content, pattern, expected) rows of the reference regex engine's `test_has_match` into a JSON fixture:

    python3 tests/golden/make_regex_cases.py <tfhe-rs checkout>

Source: tfhe/examples/regex_engine/engine.rs, the #[test_case("content", "/pattern/", 0|1 ...)] attributes above
`fn test_has_match` -> tests/golden/regex_has_match_cases.json (data only: strings and the expected bit, with the line)."""
import json
import os
import re
import sys

SOURCE = os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "tfhe", "examples", "regex_engine", "engine.rs")
text = open(SOURCE).read()
end = text.index("fn test_has_match")
start = text.rindex("lazy_static!", 0, end)
STRING = r'"((?:[^"\\]|\\.)*)"'


def unescape(s):            # Rust string literal escapes that occur in such rows
    return re.sub(r"\\(.)", lambda m: {"n": "\n", "t": "\t", "\\": "\\", '"': '"', "'": "'"}[m.group(1)], s)


rows = []
for m in re.finditer(r"#\[test_case\(%s,\s*%s,\s*([01])\b" % (STRING, STRING), text[start:end]):
    rows.append({"content": unescape(m.group(1)), "pattern": unescape(m.group(2)), "expected": int(m.group(3)),
                 "source": "tfhe/examples/regex_engine/engine.rs:%d" % (text[:start + m.start()].count("\n") + 1)})
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "regex_has_match_cases.json")
json.dump(rows, open(path, "w"), indent=1)
print(len(rows), "rows ->", path)
