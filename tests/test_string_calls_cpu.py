"""Every call of the FheString Python surface resolves to a plan that exists: over the grid of tests/string_call_grid.py
(every public operation, capacities 1 / 4 / 5, clear and encrypted operands, an empty clear pattern, a `to` of capacity 0,
out_cap absent / smaller / larger, max_parts 1..3 with and without part_cap, clear and encrypted counts), on TOY_K1 and
without a GPU.  FheStringOps._run and StringProgram.op are replaced by recorders, so nothing is executed: what is checked
is the resolution both classes share (fhestr.resolve_*)."""
import types

import pytest

import oracle as O
from conftest import to_fhestr_params
from string_call_grid import grid, operands_for_ops, operands_for_program


class _Resolved(Exception):
    pass


@pytest.fixture(scope="module")
def resolved():
    """[(call, what FheStringOps resolved it to, what StringProgram did)]: (name, a_cap, b_cap, clear, blocks of every
    operand in the plan's order), or the FheError that refused the call."""
    import fhestr
    P = to_fhestr_params(O.TOY_K1)
    ops = fhestr.FheStringOps(types.SimpleNamespace(params=P))      # resolving needs the parameters only

    def ran(name, a_cap, b_cap, clear, operands, packed=False, digits=None):
        raise _Resolved((name, a_cap, b_cap, clear, [x.shape[0] for x in operands + ([digits] if digits is not None else [])]))

    ops._run = ops._run_device = ran
    prog = fhestr.StringProgram(None, params=P)

    def recorded(name, *values, clear=None):
        caps = [v.cap for v in values if v.kind == "string"]
        raise _Resolved((name, caps[0], sum(caps[1:]), clear, [v.blocks for v in values]))

    prog.op = recorded

    def outcome(call):
        try:
            call()
        except _Resolved as e:
            return e.args[0]
        except fhestr.FheError as e:
            return e
        raise AssertionError("the call was not resolved")

    out = []
    for method, operands, kw in grid():
        for packed in (False, True):
            by_ops = outcome(lambda: getattr(ops, method)(*operands_for_ops(fhestr, P, operands), packed=packed, **kw))
            by_prog = outcome(lambda: getattr(prog, method)(*operands_for_program(prog, operands), **kw))
            out.append(((method, operands, kw, packed), by_ops, by_prog))
    prog.close()
    return out


def test_every_call_builds_or_is_refused(resolved):
    """The resolved plan builds offline and takes exactly the operands' blocks, or the call is refused with FheError --
    by the resolver, or by the builder when the plan is asked for."""
    import fhestr
    P = to_fhestr_params(O.TOY_K1)
    built, refused = {}, 0
    for call, by_ops, _ in resolved:
        if isinstance(by_ops, fhestr.FheError):
            refused += 1
            continue
        name, a_cap, b_cap, clear, blocks = by_ops
        key = (name, a_cap, b_cap, clear)
        if key not in built:
            try:
                plan = fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, params=P)
                built[key] = plan.info()["n_inputs"]
                plan.close()
            except fhestr.FheError:
                built[key] = None
        if built[key] is None:
            refused += 1
        else:
            assert built[key] == sum(blocks), (call, by_ops)
    assert refused and sum(n is not None for n in built.values()) > len(built) // 2


def test_ops_and_programs_resolve_alike(resolved):
    """FheStringOps (host and device route) and StringProgram give the same plan name, capacities, clear bytes and
    operand order for the same call.  A program has no string of capacity 0, so a `to` of capacity 0 is compared on
    FheStringOps' two routes only."""
    import fhestr
    routes = {}
    for (method, operands, kw, packed), by_ops, by_prog in resolved:
        if ("s", 0) not in operands:
            if isinstance(by_ops, fhestr.FheError):
                assert isinstance(by_prog, fhestr.FheError) and str(by_prog) == str(by_ops), (method, operands, kw)
            else:
                assert by_prog == by_ops, (method, operands, kw)
        other = routes.setdefault((method, operands, tuple(kw.items())), by_ops)
        assert str(other) == str(by_ops), (method, operands, kw)


@pytest.mark.parametrize("count", [0, 256, -1])
def test_repeat_count_is_refused_on_every_route(count):
    """A clear repeat count outside 1..255 is an FheError wherever the call would have gone."""
    import fhestr
    P = to_fhestr_params(O.TOY_K1)
    ops = fhestr.FheStringOps(types.SimpleNamespace(params=P))
    a, = operands_for_ops(fhestr, P, [("s", 4)])
    prog = fhestr.StringProgram(None, params=P)
    for call in (lambda: ops.repeat(a, count), lambda: ops.repeat(a, count, packed=True), lambda: prog.repeat(prog.string(4), count)):
        with pytest.raises(fhestr.FheError, match="count must be in 1..255"):
            call()
    prog.close()


def test_empty_from_is_refused_on_every_route():
    """An encrypted `from` of capacity 0 (general replace, replacen) is an FheError before any plan is asked for."""
    import fhestr
    P = to_fhestr_params(O.TOY_K1)
    ops = fhestr.FheStringOps(types.SimpleNamespace(params=P))
    a, frm, to, n = operands_for_ops(fhestr, P, [("s", 4), ("s", 0), ("s", 1), ("n", 3)])
    for packed in (False, True):
        for call in (lambda: ops.replace(a, frm, to, out_cap=4, packed=packed), lambda: ops.replacen(a, frm, to, 1, packed=packed),
                     lambda: ops.replacen(a, frm, to, n, packed=packed)):
            with pytest.raises(fhestr.FheError, match="`from` needs a capacity of at least one character"):
                call()
