"""One list of oc_potential and oc_featurize calls, each there for ONE kernel instance, the states they start from, and the C
oracle's answer.

The family launches four kernel instances (csrc/derived_dispatch.hpp: oc_potential, launch_featurize): k_potential2 (every layout of the
table has one or two pots), k_potential (any other table, and withheld hints), k_featurize<LAY_LDS=true> (a table of at most 32
layouts) and k_featurize<LAY_LDS=false>.  Every case names the instance it is there for (`expect`: the words of oc_potential_plan /
oc_featurize_plan up to and including the instance's name); tests/test_host_derived_instances.py holds the list to the planner's
answers and to the instances the sources launch, without a GPU, and tests/test_gpu_derived_instances.py runs every case against
the oracle at zero tolerance (phi is float64 built from table entries in the reference's operand order, features are small
integers).

The default batch is 2 307 envs = 9 * 256 + 3: for oc_potential ten workgroups with a last wavefront of 3 lanes, for oc_featurize
18 whole blocks of 128 envs and one of 3.

The states are `directed_states`: helpers.random_packed_states (valid states: players on distinct floor cells — unreachable ones
included, as on forced_coordination —, random hands, counters and pots), over which every env draws ONE named situation from the
short list its layout can hold (`applicable`) and gets its pots, hands and, where the situation is about motion costs, its players'
cells rewritten for it; everything else stays random.  `census(case)` counts, from the states and the host planner's cost tables
alone, the envs in which each situation holds (a situation also counts where the random part of another env happens to produce
it).  Every situation a case lists (`Case.situations`) holds in at least FLOOR = 64 envs of the batch, one wavefront's worth, and
at least once in every whole 256-env workgroup (the last group of a 2 307-env batch has 3 envs: it cannot hold a dozen
situations, and is held to none).  A situation a layout cannot produce is not listed by the cases on it.

The situations of phi (potential_function, mdp.py:2920-3238; csrc/potential.hpp):
  set_order_matters      two or more partially full pots share the best sort_value among the partially full ones, exactly one
                         player holds an ingredient, both of the first two of those pots (in the order of
                         `list(set().union(...))`) miss it, and that player's capped costs min(cost, pot_*_steps) to the two
                         differ: phi depends on which pot the set hands over first
  set_order_two_then_one (two-pot layouts) slot 0 holds two items, slot 1 one, one holder of an ingredient both miss: the insertion
                         order (B, A), which reads the record's second order bit (where the sort_values of the two differ, the
                         stable sort decides after the bit is read)
  set_order_bit1_tie     (two-pot layouts whose orders leave some soups worthless) slot 0 holds two items, slot 1 one, both soups
                         worth nothing whatever is added (sort_value 0.0 twice: the second order bit decides), an empty-handed
                         player, and different capped distances min(cook_dist, max_pickup_steps) to the two: their terms differ,
                         and the order in which phi adds them is the set's
  three_or_four_partial  set_order_matters with three or four partially full pots: more than two, the 8-slot set not yet resized
  set_resize             set_order_matters with five or more: the set grows to 32 slots at the fifth insert
  set_resize_all_eight   ... with all eight pots partially full
  ready_before_cooking   slot 0 ready, slot 1 cooking, a dish in some hand (k_potential2's swap_ni)
  two_dishes_two_soups   both players hold a dish, two pots are cooking or ready;  two_dishes_same_soup: ... and prefer the same one
  dish_unreachable       a dish holder whose every cooking or ready pot is at infinite cost
  soup_in_hand           a held soup;  soup_unservable: its holder reaches no serving cell
  full_idle_free_hand    a three-item pot that is not cooking and an empty-handed player;  full_idle_no_free_hand: ... and none
                         (cook_dist infinite)
  leftover_both_kinds    no partially full pot, an onion holder and a tomato holder, an empty pot both reach
  leftover_no_empty_pot  no partially full pot, an ingredient holder, no empty pot (adds 0.0)
  long_cook / short_cook a cooking pot with more / at most max_pickup_steps left
  mixed_completion       a partially full pot whose best completion adds both kinds
and of the features (featurize_state, mdp.py:2579-2898; csrc/featurize.hpp), `pN` = the player the feature row belongs to:
  held_<kind>_p<N>       each of onion, tomato, dish, soup in each hand
  pot<r>_<class>         the pot player 0's walk record ranks r-th (r <= num_pots) is empty / idle1 / idle2 / idle3 / cooking / ready;
                         pot3_absent, pot4_absent: the record has no such pot (the zero block)
  counter_beats_dispenser  with counters as motion goals: an onion / tomato / dish on a counter strictly cheaper to reach than the
                         closest dispenser of its kind, for a player not holding that kind;  counter_ties_dispenser: equally cheap,
                         nothing of the kind cheaper (the dispenser group wins)
  counter_soup           a reachable soup on a goal counter;  counter_soup_tomato: one with tomatoes in it
  nearest_counter_taken  the first goal counter of a player's sorted list is occupied
  counter_unreachable    an object on a counter that is no goal of, or out of reach for, some player (cost 255)
"""
import functools
from collections import namedtuple

import numpy as np

import train_cases  # noqa: F401 (its tables and rollout_cases': the import registers them)
from case_support import env_layout_ids, layout_ids, new_oracle, register_grid, register_table, table_of
from helpers import random_packed_states
from rollout_cases import SEVEN

N_ENVS = 2307  # 9 * 256 + 3 = 18 * 128 + 3
GAMMAS = (0.99, 0.9)
FLOOR, GROUP = 64, 256
INSTANCES = ("k_potential2", "k_potential", "k_featurize<LAY_LDS=true>", "k_featurize<LAY_LDS=false>")
# Instances no call reaches, each with its reason: none — every instance has a case
UNREACHABLE = {}
THREE_POTS = "XPPPX\nO 2 T\nX1  X\nXDXSX"  # cramped_room's size, three pots in one row, tomatoes; the bonus order makes oot the best soup
EIGHT_POTS_SERVE_RING = "XPPPPPPPPX\nO  1   2 T\nS        S\nS        S\nS        S\nS        S\nS        S\nS        S\nSDSSSSSSSS"
ONE_PLAYER_TWO_POTS = "XPPXX\nO   O\nX1  X\nXDXSX"  # train_cases' cramped_room_two_pots without player 2
INF = 1 << 20
EMPTY, COOKING, READY = 0, 4, 5  # pot classes as csrc/potential.hpp names them; 1..3 = idle with that many items
KINDS = (("onion", 1), ("tomato", 2), ("dish", 3), ("soup", 0x80))
POT_CLASSES = ("empty", "idle1", "idle2", "idle3", "cooking", "ready")

Case = namedtuple("Case", "id table kind expect n_envs hints num_pots counter_goals situations seed env_offset")


def case(id, table, expect, situations, n_envs=N_ENVS, hints=True, num_pots=None, counter_goals=None, seed=None, env_offset=None):
    """kind: "potential" (num_pots None: run at every gamma of GAMMAS) or "featurize" (num_pots 0..4; counter_goals "none", "all" or
    "half": the list of every counter (x, y) with x + y even, about half of each layout's); hints: False withholds max_pots,
    batch_flags and max_free_cells; situations: what the case's states are held to (see the module's text)."""
    k = len(CASES)
    kind = "potential" if num_pots is None else "featurize"
    assert (kind == "featurize") == (counter_goals is not None) and expect in INSTANCES
    c = Case(id, table, kind, expect, n_envs, hints, num_pots, counter_goals, tuple(situations), 301 + k if seed is None else seed,
             5 * n_envs + 64 * k + 11 if env_offset is None else env_offset)
    CASES.append(c)
    return c


# the situations, by what a layout needs for them
_ANY = ("soup_in_hand", "full_idle_free_hand", "full_idle_no_free_hand", "leftover_no_empty_pot", "long_cook", "short_cook")
_TWO_PLAYERS = ("leftover_both_kinds",)
_TWO_POTS = ("set_order_matters", "ready_before_cooking")
_TWO_OF_EACH = ("two_dishes_two_soups", "two_dishes_same_soup")
_BITS = ("set_order_two_then_one", "set_order_bit1_tie")  # two-pot layouts whose orders leave tomato soups worthless
_HELD = tuple("held_%s_p%d" % (k, p) for k, _ in KINDS for p in (0, 1))
_COUNTERS = ("counter_beats_dispenser", "counter_ties_dispenser", "counter_soup", "nearest_counter_taken")


def _pots(r_max, absent=()):
    return tuple("pot%d_%s" % (r, cl) for r in range(1, r_max + 1) if r not in absent for cl in POT_CLASSES) + tuple("pot%d_absent" % r for r in absent)


CASES = []
# ---- k_potential2: every layout with one or two pots
case("potential2_one_pot", "cramped_room", "k_potential2", _ANY + _TWO_PLAYERS)  # (pot B absent)
case("potential2_two_pots", "asymmetric_advantages", "k_potential2", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + _BITS,
     seed=290, env_offset=4001)  # (W = 9)
case("potential2_unreachable", "forced_coordination_tomato", "k_potential2",  # (infinite costs, tomatoes)
     _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("set_order_two_then_one", "dish_unreachable", "soup_unservable"))
case("potential2_other_constants", "mdp_test_tomato", "k_potential2",  # (POTENTIAL_CONSTANTS 4/4/5/6)
     _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("set_order_two_then_one", "mixed_completion"))
case("potential2_serve_scan", "you_shall_not_pass", "k_potential2",  # (16 serving cells: the terrain scan)
     _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("set_order_two_then_one", "mixed_completion"))
case("potential2_one_player_two_pots", "one_player_two_pots", "k_potential2", _ANY + _TWO_POTS + _BITS)
case("potential2_126_cells", "corridor", "k_potential2", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + _BITS)  # (row stride 128)
# (one- and two-pot lanes in a wavefront, padded 9 x 5)
case("potential2_mixed_table", "mix5", "k_potential2", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + _BITS + ("dish_unreachable", "soup_unservable"))
case("potential2_forty_layouts", "canonical_5_x8", "k_potential2", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + _BITS + ("dish_unreachable", "soup_unservable"))
# ---- k_potential: withheld hints (max_pots == 0) on tables k_potential2 serves, then three to eight pots
case("potential_hints_withheld", "asymmetric_advantages", "k_potential", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + _BITS,
     hints=False, seed=290, env_offset=4001)  # (the states of potential2_two_pots)
case("potential_hints_withheld_one_pot", "cramped_room", "k_potential", _ANY + _TWO_PLAYERS, hints=False)
case("potential_three_pots", "three_pots", "k_potential", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("three_or_four_partial", "mixed_completion"))
case("potential_seven_pots", "seven_pots", "k_potential", _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("three_or_four_partial", "set_resize"))
case("potential_eight_pots_serve_scan", "eight_pots_serve_ring", "k_potential",  # (the resize, the terrain scan, 90 cells)
     _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("three_or_four_partial", "set_resize", "set_resize_all_eight"))
case("potential_mixed_with_seven", "seven_and_scenario2_s", "k_potential",  # (1-, 2- and 7-pot lanes, padded 7 x 4)
     _ANY + _TWO_PLAYERS + _TWO_POTS + _TWO_OF_EACH + ("three_or_four_partial", "set_resize", "set_order_bit1_tie"))
# ---- k_featurize<LAY_LDS=true>
case("featurize_one_pot", "cramped_room", "k_featurize<LAY_LDS=true>", _HELD + _pots(2, absent=(2,)), num_pots=2, counter_goals="none")
case("featurize_no_pot_blocks", "asymmetric_advantages", "k_featurize<LAY_LDS=true>", _HELD + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"),
     num_pots=0, counter_goals="all")
case("featurize_unreachable", "forced_coordination", "k_featurize<LAY_LDS=true>", _HELD + _pots(2) + ("pot1_absent", "pot2_absent") + _COUNTERS + ("counter_unreachable",),
     num_pots=2, counter_goals="all")  # (a player who reaches no pot: both blocks zero)
case("featurize_three_of_four_pots", "three_pots", "k_featurize<LAY_LDS=true>", _HELD + _pots(4, absent=(4,)) + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"),
     num_pots=4, counter_goals="all")  # (a real third block and a zero fourth)
case("featurize_eight_pots", "eight_pots_serve_ring", "k_featurize<LAY_LDS=true>", _HELD + _pots(4) + ("counter_unreachable",), num_pots=4, counter_goals="all")  # (84 992 B LDS; its two counters are corners: no goals)
case("featurize_largest_lds", "corridor", "k_featurize<LAY_LDS=true>", _HELD + _pots(4, absent=(3, 4)) + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"), num_pots=4,
     counter_goals="all")  # (9 planes: 89 088 B)
case("featurize_counter_list", "mix5", "k_featurize<LAY_LDS=true>", _HELD + _pots(2) + ("pot1_absent", "pot2_absent") + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"),
     num_pots=2, counter_goals="half")
case("featurize_mixed_with_seven", "seven_and_scenario2_s", "k_featurize<LAY_LDS=true>", _HELD + _pots(3) + ("pot2_absent", "pot3_absent") + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"),
     num_pots=3, counter_goals="all")
# ---- k_featurize<LAY_LDS=false>: a table of more than 32 layouts
case("featurize_forty_layouts_none", "canonical_5_x8", "k_featurize<LAY_LDS=false>", _HELD + _pots(2) + ("pot1_absent", "pot2_absent"), num_pots=2,
     counter_goals="none")
case("featurize_forty_layouts_all", "canonical_5_x8", "k_featurize<LAY_LDS=false>", _HELD + _pots(2) + ("pot1_absent", "pot2_absent") + _COUNTERS + ("counter_soup_tomato", "counter_unreachable"),
     num_pots=2, counter_goals="all")
# ---- the copy-out's edges: one env, one short of a block, one more than a block (no census: fewer than FLOOR envs per situation)
for _n in (1, 127, 129):
    case("featurize_%d_env%s" % (_n, "" if _n == 1 else "s"), "cramped_room", "k_featurize<LAY_LDS=true>", (), n_envs=_n, num_pots=2, counter_goals="all")
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def _table(name):
    from overcooked_ai_amd.layouts import LayoutSpec, LayoutTable, spec_from_name

    if name == "three_pots":
        oot = {"ingredients": ["onion", "onion", "tomato"]}
        return LayoutTable([LayoutSpec(dict(grid=THREE_POTS, layout_name=name, start_bonus_orders=[oot],
                                            start_all_orders=[{"ingredients": ["onion"] * 3}, oot, {"ingredients": ["tomato"] * 3}]))])
    if name == "eight_pots_serve_ring":
        return LayoutTable([LayoutSpec(dict(SEVEN, grid=EIGHT_POTS_SERVE_RING, layout_name=name))])
    assert name == "mdp_test_tomato"  # the registry's mdp_test under the name the second set of POTENTIAL_CONSTANTS is keyed by
    return LayoutTable([LayoutSpec(dict(spec_from_name("mdp_test").to_layout_dict(), layout_name=name))])


# this list's own tables
for _name in ("three_pots", "eight_pots_serve_ring", "mdp_test_tomato"):
    register_table(_name, functools.partial(_table, _name))
register_grid("one_player_two_pots", ONE_PLAYER_TWO_POTS)


def counter_goals_of(c):
    """What the case hands to VecOvercookedEnv.featurize as counter_goals: "none", "all", or the list of "half"."""
    if c.counter_goals != "half":
        return c.counter_goals
    table = table_of(c.table)
    return sorted({(x, y) for s in table.specs for (x, y) in s.cells_of("X") if (x + y) % 2 == 0})


# ------------------------------------------------------------------------------------------ what a layout gives
class _Ctx:
    """A layout as the situations need it: its cells, the host planner's costs (planner.feature_costs: 255 = out of reach, +1 for
    the interact), its walk records, and potential.py's record of the best completions."""

    def __init__(self, spec, goals):
        import struct

        from overcooked_ai_amd import planner
        from overcooked_ai_amd.potential import phi_record, potential_params

        self.spec, self.W = spec, spec.width
        cell = lambda xy: xy[1] * spec.width + xy[0]  # noqa: E731
        self.floor = [cell(p) for p in spec.cells_of(" ")]
        self.pots = [cell(p) for p in spec.cells_of("P")]
        self.serve = [cell(p) for p in spec.cells_of("S")]
        self.counters = [cell(p) for p in spec.cells_of("X")]
        self.disp = {1: [cell(p) for p in spec.cells_of("O")], 2: [cell(p) for p in spec.cells_of("T")], 3: [cell(p) for p in spec.cells_of("D")]}
        self.np, self.has_tomato = spec.num_players, bool(spec.cells_of("T"))
        self.fidx, self.cost = planner.feature_costs(spec, goals)
        self.goals_on = goals != "none"
        self.walk = planner.walk_records(spec, self.cost)[0]
        p = potential_params(spec, 0.99)
        self.max_del, self.max_pick = p["max_delivery_steps"], p["max_pickup_steps"]
        self.steps = {1: p["pot_onion_steps"], 2: p["pot_tomato_steps"]}
        recs = [phi_record(spec, g) for g in GAMMAS]
        self.sort_value = [tuple(struct.unpack_from("<16d", r, 40)[k] for r in recs) for k in range(16)]
        self.value_max1 = struct.unpack_from("<16d", recs[0], 296)
        self.pw = struct.unpack_from("<512d", recs[0], 472)
        self.opt = {}  # (n_o, n_t) -> (missing onions, missing tomatoes) of the best completion
        for n_t in range(4):
            for n_o in range(4 - n_t):
                if n_o + n_t:
                    ok = recs[0][424 + n_o + 4 * n_t]
                    self.opt[(n_o, n_t)] = ((ok & 3) - n_o, (ok >> 2) - n_t)
        self.keys = [k for k in self.opt if self.has_tomato or k[1] == 0]
        # (two items, one item) soups that tie at a sort_value of 0.0 and miss nothing: nothing added makes them worth anything
        self.tie_pairs = [(a, b) for a in self.opt for b in self.opt if sum(a) == 2 and sum(b) == 1 and self.opt[a] == (0, 0) == self.opt[b]
                          and self.sort_value[a[0] + 4 * a[1]] == self.sort_value[b[0] + 4 * b[1]]]
        self.mixed_keys = [k for k in self.keys if sum(k) < 3 and self.opt[k][0] > 0 and self.opt[k][1] > 0]
        # per floor cell: the pots and whether a serving cell can be reached from it (orientation changes no reachability)
        self.reach_pot = {f: [self.cost[4 * self.fidx[f], c] != 255 for c in self.pots] for f in self.floor}
        self.reach_serve = {f: any(self.cost[4 * self.fidx[f], c] != 255 for c in self.serve) for f in self.floor}

    def c(self, pos, ori, cell):
        v = int(self.cost[4 * int(self.fidx[pos]) + ori, cell])
        return INF if v == 255 else v + 1

    def time(self, key):
        return int(self.spec.recipe_time(key))


_CTX = {}


def _ctx(spec, goals):
    key = (id(spec), goals if isinstance(goals, str) else tuple(goals))
    if key not in _CTX:
        _CTX[key] = _Ctx(spec, goals)
    return _CTX[key]


def applicable(ctx, kind, num_pots=2):
    """The situations `directed_states` draws from on this layout, each as often as it is named."""
    n_pots = len(ctx.pots)
    if kind == "featurize":
        names = ["plain"]
        if ctx.goals_on:
            names += list(_COUNTERS) + (["counter_soup_tomato"] if ctx.has_tomato else [])
            if any((ctx.cost[:, c] == 255).any() for c in ctx.counters):
                names.append("counter_unreachable")
        return names
    names = [n for n in _ANY if n != "long_cook" or any(ctx.time(k) > ctx.max_pick for k in ctx.keys)]
    if ctx.np == 2:
        names += list(_TWO_PLAYERS)
    if n_pots >= 2:
        names += list(_TWO_POTS) + (list(_TWO_OF_EACH) if ctx.np == 2 else [])
    if n_pots == 2:
        names += ["set_order_matters", "set_order_two_then_one"] + (["set_order_bit1_tie"] * 2 if ctx.tie_pairs else [])
    if n_pots >= 3:
        names += ["three_or_four_partial"] * 2
    if n_pots >= 5:
        names += ["set_resize"] * 4
    if n_pots == 8:
        names += ["set_resize_all_eight"] * 2
    if any(not all(r) for r in ctx.reach_pot.values()):
        names += ["dish_unreachable"] * 2
    if not all(ctx.reach_serve.values()):
        names += ["soup_unservable"] * 2
    if ctx.mixed_keys:
        names.append("mixed_completion")
    return names


# ------------------------------------------------------------------------------------------ writing a situation into an env
def _soup_code(key, rng):
    n = key[0] + key[1]
    bits = 0
    for b in rng.permutation(n)[:key[1]]:
        bits |= 1 << int(b)
    return 0x80 | (n << 3) | bits


def _set_pot(ctx, st, e, k, key, mode, rng, rem=None):
    """mode: "empty", "idle", "cooking" (rem steps left, drawn when None) or "ready" """
    c = ctx.pots[k]
    if mode == "empty":
        st[1 + (c >> 4), e, c & 15], st[0, e, 8 + k] = 0, 0
        return
    ct = ctx.time(key)
    if mode == "cooking" and rem is None:
        rem = int(rng.integers(1, ct + 1))
    st[1 + (c >> 4), e, c & 15] = _soup_code(key, rng)
    st[0, e, 8 + k] = 0 if mode == "idle" else ct + 1 if mode == "ready" else ct - rem + 1


def _rand_key(ctx, rng, n=None):
    n = int(rng.integers(1, 4)) if n is None else n
    n_t = int(rng.integers(0, n + 1)) if ctx.has_tomato else 0
    return (n - n_t, n_t)


def _not_partial(ctx, st, e, k, rng, empty_ok=True):
    """pot k: empty, full and idle, cooking or ready"""
    mode = ("empty", "idle", "cooking", "ready")[int(rng.integers(0 if empty_ok else 1, 4))]
    _set_pot(ctx, st, e, k, _rand_key(ctx, rng, 3 if mode == "idle" else None), mode, rng)


def _hand(st, e, p, obj):
    st[0, e, 3 * p + 2] = obj


def _other_hand(ctx, st, e, p, rng):
    """player p (if there is one) holds nothing, a dish or a soup: no ingredient"""
    if p < ctx.np:
        _hand(st, e, p, (0, 3, _soup_code(_rand_key(ctx, rng), rng))[int(rng.integers(0, 3))])


def _place(ctx, st, e, rng, ok=None, tries=60):
    """The players on distinct floor cells with random orientations, redrawn until ok([(cell, orientation), ...]) holds."""
    for _ in range(tries):
        cells = rng.choice(len(ctx.floor), size=ctx.np, replace=False)
        who = [(ctx.floor[int(c)], int(rng.integers(0, 4))) for c in cells]
        if ok is None or ok(who):
            for p, (cell, ori) in enumerate(who):
                st[0, e, 3 * p], st[0, e, 3 * p + 1] = cell, ori
            return True
    return False


def _place_at(ctx, st, e, rng, h, f):
    """Player h on floor cell f, the other one on any other."""
    _place(ctx, st, e, rng)
    others = [c for c in ctx.floor if c != f]
    for p in range(ctx.np):
        st[0, e, 3 * p] = f if p == h else others[int(rng.integers(0, len(others)))]


def _players(ctx, st, e):
    return [(int(st[0, e, 3 * p]), int(st[0, e, 3 * p + 1]), int(st[0, e, 3 * p + 2])) for p in range(ctx.np)]


def _partial_pots(ctx, st, e, rng, which, two_then_one=False):
    """The pots `which` partially full with one key (two_then_one: two items in the first, one in the second), every other pot
    not partially full; one player holds an ingredient all of them miss, the other none; the holder stands where its capped costs
    to the first two pots the set hands over differ (where the layout has such a place)."""
    from overcooked_ai_amd.potential import py_set_order

    for _ in range(20):
        key = _rand_key(ctx, rng, int(rng.integers(1, 3)))
        keys = [key] * len(which)
        if two_then_one:  # a two-item key and the one-item key under it
            key = _rand_key(ctx, rng, 2)
            keys = [key, (key[0] - 1, key[1]) if key[0] and (not key[1] or rng.random() < 0.5) else (key[0], key[1] - 1)]
        kinds = [i for i in (1, 2) if all(ctx.opt[k][i - 1] > 0 for k in keys)]
        if kinds:
            break
    else:
        return
    ing = kinds[int(rng.integers(0, len(kinds)))]
    for k in range(len(ctx.pots)):
        if k in which:
            _set_pot(ctx, st, e, k, keys[which.index(k)], "idle", rng)
        else:
            _not_partial(ctx, st, e, k, rng)
    h = int(rng.integers(0, ctx.np))
    _hand(st, e, h, ing)
    _other_hand(ctx, st, e, 1 - h, rng)
    ins = sorted(which, key=lambda k: (sum(keys[which.index(k)]), k))  # one-item pots, then two-item pots, each in pot order
    order = py_set_order([(ctx.pots[k] % ctx.W, ctx.pots[k] // ctx.W) for k in ins])
    a, b = (y * ctx.W + x for (x, y) in order[:2])
    cap = ctx.steps[ing]
    _place(ctx, st, e, rng, lambda who: min(ctx.c(who[h][0], who[h][1], a), cap) != min(ctx.c(who[h][0], who[h][1], b), cap))


def _choose(rng, n, m):
    return sorted(int(k) for k in rng.choice(n, size=m, replace=False))


def _write_potential(name, ctx, st, e, rng):
    n_pots = len(ctx.pots)
    if name == "set_order_matters":
        _partial_pots(ctx, st, e, rng, _choose(rng, n_pots, 2))
    elif name == "set_order_two_then_one":
        _partial_pots(ctx, st, e, rng, [0, 1], two_then_one=True)
    elif name == "set_order_bit1_tie":
        two, one = ctx.tie_pairs[int(rng.integers(0, len(ctx.tie_pairs)))]
        _set_pot(ctx, st, e, 0, two, "idle", rng)
        _set_pot(ctx, st, e, 1, one, "idle", rng)
        h = int(rng.integers(0, ctx.np))
        _hand(st, e, h, 0)
        _other_hand(ctx, st, e, 1 - h, rng)
        _place(ctx, st, e, rng, lambda who: len(set(_cook_dists(ctx, st, e, who))) == 2)
    elif name == "three_or_four_partial":
        _partial_pots(ctx, st, e, rng, _choose(rng, n_pots, min(n_pots, int(rng.integers(3, 5)))))
    elif name == "set_resize":
        _partial_pots(ctx, st, e, rng, _choose(rng, n_pots, int(rng.integers(5, n_pots + 1))))
    elif name == "set_resize_all_eight":
        _partial_pots(ctx, st, e, rng, list(range(8)))
    elif name == "ready_before_cooking":
        _set_pot(ctx, st, e, 0, _rand_key(ctx, rng), "ready", rng)
        _set_pot(ctx, st, e, 1, _rand_key(ctx, rng), "cooking", rng)
        _hand(st, e, int(rng.integers(0, ctx.np)), 3)
    elif name in ("two_dishes_two_soups", "two_dishes_same_soup"):
        a, b = _choose(rng, n_pots, 2)
        for p in range(ctx.np):
            _hand(st, e, p, 3)
        if name == "two_dishes_two_soups":
            for k in (a, b):
                _set_pot(ctx, st, e, k, _rand_key(ctx, rng), ("cooking", "ready")[int(rng.integers(0, 2))], rng)
        else:  # one soup ready, every other pot idle or empty: whoever reaches it prefers it
            for k in range(n_pots):
                _set_pot(ctx, st, e, k, _rand_key(ctx, rng), "idle" if rng.random() < 0.5 else "empty", rng)
            _set_pot(ctx, st, e, a, _rand_key(ctx, rng), "ready", rng)
            _set_pot(ctx, st, e, b, _rand_key(ctx, rng), "cooking", rng)
            _place(ctx, st, e, rng, lambda who: _same_soup(ctx, st, e, who))
    elif name == "dish_unreachable":
        cells = [f for f in ctx.floor if not all(ctx.reach_pot[f])]
        f = cells[int(rng.integers(0, len(cells)))]
        h = int(rng.integers(0, ctx.np))
        _place_at(ctx, st, e, rng, h, f)
        _hand(st, e, h, 3)
        far = [k for k in range(n_pots) if not ctx.reach_pot[f][k]]
        for k in range(n_pots):
            if k in far and (k == far[0] or rng.random() < 0.5):
                _set_pot(ctx, st, e, k, _rand_key(ctx, rng), ("cooking", "ready")[int(rng.integers(0, 2))], rng)
            elif k not in far:
                _set_pot(ctx, st, e, k, _rand_key(ctx, rng), "idle" if rng.random() < 0.5 else "empty", rng)
    elif name in ("soup_in_hand", "soup_unservable"):
        h = int(rng.integers(0, ctx.np))
        _hand(st, e, h, _soup_code(_rand_key(ctx, rng), rng))
        if name == "soup_unservable":
            cells = [f for f in ctx.floor if not ctx.reach_serve[f]]
            _place_at(ctx, st, e, rng, h, cells[int(rng.integers(0, len(cells)))])
    elif name in ("full_idle_free_hand", "full_idle_no_free_hand"):
        _set_pot(ctx, st, e, int(rng.integers(0, n_pots)), _rand_key(ctx, rng, 3), "idle", rng)
        for p in range(ctx.np):
            _hand(st, e, p, (1, 2, 3, _soup_code(_rand_key(ctx, rng), rng))[int(rng.integers(0, 4))])
        if name == "full_idle_free_hand":
            _hand(st, e, int(rng.integers(0, ctx.np)), 0)
    elif name in ("leftover_both_kinds", "leftover_no_empty_pot"):
        for k in range(n_pots):
            _not_partial(ctx, st, e, k, rng, empty_ok=name == "leftover_both_kinds")
        h = int(rng.integers(0, ctx.np))
        _hand(st, e, h, int(rng.integers(1, 3)))
        if name == "leftover_both_kinds":
            _hand(st, e, h, 1)
            _hand(st, e, 1 - h, 2)
            k = int(rng.integers(0, n_pots))
            _set_pot(ctx, st, e, k, None, "empty", rng)
            _place(ctx, st, e, rng, lambda who: all(ctx.reach_pot[f][k] for f, _ in who))
    elif name in ("long_cook", "short_cook"):
        keys = [k for k in ctx.keys if ctx.time(k) > ctx.max_pick] if name == "long_cook" else ctx.keys
        key = keys[int(rng.integers(0, len(keys)))]
        ct = ctx.time(key)
        rem = int(rng.integers(ctx.max_pick + 1, ct + 1)) if name == "long_cook" else int(rng.integers(1, min(ct, ctx.max_pick) + 1))
        _set_pot(ctx, st, e, int(rng.integers(0, n_pots)), key, "cooking", rng, rem=rem)
    elif name == "mixed_completion":
        _set_pot(ctx, st, e, int(rng.integers(0, n_pots)), ctx.mixed_keys[int(rng.integers(0, len(ctx.mixed_keys)))], "idle", rng)
    else:
        raise KeyError(name)


def _cook_dists(ctx, st, e, who):
    """min(cook_dist, max_pickup_steps) to either pot of a two-pot layout: cook_dist over the empty-handed players (mdp.py:3192-3203)"""
    free = [w for p, w in enumerate(who) if st[0, e, 3 * p + 2] == 0]
    return [min([ctx.c(w[0], w[1], c) for w in free] + [ctx.max_pick]) for c in ctx.pots[:2]]


def _pot_view(ctx, st, e):
    """[(class, key, steps left)] per pot slot, as get_pot_states sorts them (mdp.py:1809-1838)"""
    out = []
    for k, c in enumerate(ctx.pots):
        o, tk = int(st[1 + (c >> 4), e, c & 15]), int(st[0, e, 8 + k])
        if o == 0:
            out.append((EMPTY, None, 0))
            continue
        n, n_t = (o >> 3) & 3, bin(o & 7).count("1")
        key, ct = (n - n_t, n_t), ctx.time((n - n_t, n_t))
        cls = n if tk == 0 else READY if tk - 1 >= ct else COOKING
        out.append((cls, key, ct - (tk - 1) if cls == COOKING else 0))
    return out


def _preferred(ctx, pots, pos, ori):
    """The index, among the cooking-then-ready pots, of the soup a dish holder at (pos, ori) pursues; -1: none (mdp.py:3092-3133)"""
    ni = [k for cls in (COOKING, READY) for k, p in enumerate(pots) if p[0] == cls]
    best, best_value = -1, 0.0
    for i, k in enumerate(ni):
        d = ctx.c(pos, ori, ctx.pots[k])
        value = ctx.pw[max(pots[k][2], min(d, ctx.max_pick))] * (ctx.pw[ctx.max_del] * ctx.value_max1[pots[k][1][0] + 4 * pots[k][1][1]])
        if d != INF and value > best_value:
            best, best_value = i, value
    return best


def _same_soup(ctx, st, e, who):
    pots = _pot_view(ctx, st, e)
    first = _preferred(ctx, pots, *who[0])
    return first >= 0 and all(_preferred(ctx, pots, *w) == first for w in who[1:])


def _counter_cost(ctx, who, c):
    return int(ctx.cost[4 * int(ctx.fidx[who[0]]) + who[1], c])


def _dispenser_cost(ctx, who, kind):
    return min([_counter_cost(ctx, who, c) for c in ctx.disp[kind]] or [255])


def _write_featurize(name, ctx, st, e, rng, h):
    """Every env: pot classes drawn evenly, the hands cycling through (nothing, onion, tomato, dish, soup)^2; then the counter
    situation `name` for one player."""
    for k in range(len(ctx.pots)):
        cl = int(rng.integers(0, 6))
        mode = ("empty", "idle", "idle", "idle", "cooking", "ready")[cl]
        _set_pot(ctx, st, e, k, _rand_key(ctx, rng, cl if 1 <= cl <= 3 else None), mode, rng)
    for p in range(ctx.np):
        kind = (h // (5 if p else 1)) % 5
        _hand(st, e, p, 0 if kind == 0 else _soup_code(_rand_key(ctx, rng), rng) if kind == 4 else KINDS[kind - 1][1])
    if name == "plain":
        return
    put = lambda c, o: st.__setitem__((1 + (c >> 4), e, c & 15), o)  # noqa: E731
    p = int(rng.integers(0, ctx.np))
    if name in ("counter_beats_dispenser", "counter_ties_dispenser"):
        kinds = [k for k in (1, 2, 3) if ctx.disp[k]]
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if int(st[0, e, 3 * p + 2]) == kind:
            _hand(st, e, p, 0)
        tie = name == "counter_ties_dispenser"
        found = []

        def ok(who):
            d = _dispenser_cost(ctx, who[p], kind)
            found[:] = [c for c in ctx.counters if d != 255 and (_counter_cost(ctx, who[p], c) == d if tie else _counter_cost(ctx, who[p], c) < d)]
            return bool(found)

        if ok([(int(st[0, e, 3 * q]), int(st[0, e, 3 * q + 1])) for q in range(ctx.np)]) or _place(ctx, st, e, rng, ok):
            if tie:  # nothing of the kind cheaper than the dispenser
                who = (int(st[0, e, 3 * p]), int(st[0, e, 3 * p + 1]))
                d = _dispenser_cost(ctx, who, kind)
                for c in ctx.counters:
                    if int(st[1 + (c >> 4), e, c & 15]) == kind and _counter_cost(ctx, who, c) < d:
                        put(c, 0)
            put(found[int(rng.integers(0, len(found)))], kind)
        return
    who = (int(st[0, e, 3 * p]), int(st[0, e, 3 * p + 1]))
    near = sorted((_counter_cost(ctx, who, c), c) for c in ctx.counters if _counter_cost(ctx, who, c) != 255)
    if name in ("counter_soup", "counter_soup_tomato") and near:
        key = _rand_key(ctx, rng)
        if name == "counter_soup_tomato" and key[1] == 0:
            key = (key[0] - 1, 1) if key[0] > 1 else (0, 1)
        put(near[int(rng.integers(0, len(near)))][1], _soup_code(key, rng))
    elif name == "nearest_counter_taken" and near:
        put(near[0][1], (1, 2, 3, _soup_code(_rand_key(ctx, rng), rng))[int(rng.integers(0, 4))])
    elif name == "counter_unreachable":
        far = [c for c in ctx.counters if _counter_cost(ctx, who, c) == 255]
        if far:
            put(far[int(rng.integers(0, len(far)))], (1, 2, 3, _soup_code(_rand_key(ctx, rng), rng))[int(rng.integers(0, 4))])


def directed_states(spec, n, rng, kind="potential", counter_goals="none", first=0):
    """uint8 [n_planes, n, 16]: n valid packed states of `spec` — helpers.random_packed_states, over which env j holds the situation
    applicable(...)[(first + j) % len] (the module's text says what each one is)."""
    st = random_packed_states(spec, n, rng)
    ctx = _ctx(spec, counter_goals)
    names = applicable(ctx, kind)
    for j in range(n):
        name = names[(first + j) % len(names)]
        if kind == "potential":
            _write_potential(name, ctx, st, j, rng)
        else:
            _write_featurize(name, ctx, st, j, rng, (first + j) // len(names) + first)
    return st


@functools.lru_cache(maxsize=None)
def _states(table_name, n_envs, seed, env_offset, kind, goals):
    table = table_of(table_name)
    K = len(table)
    lid = env_layout_ids(n_envs, env_offset, K)
    rng = np.random.default_rng(seed)
    goals = goals if isinstance(goals, str) else list(goals)
    if lid is None:
        st = directed_states(table.specs[0], n_envs, rng, kind, goals)
    else:
        st = np.zeros((table.n_planes, n_envs, 16), np.uint8)
        for l in range(K):
            idx = np.nonzero(lid == l)[0]
            st[:, idx] = directed_states(table.specs[l], len(idx), rng, kind, goals, first=7 * l)
    st.setflags(write=False)
    return st


def states_of(c):
    """uint8 [n_planes, n_envs, 16], read-only: the states the call is made on (computed once per table, batch, seed and kind)."""
    goals = counter_goals_of(c) if c.kind == "featurize" else "none"
    return _states(c.table, c.n_envs, c.seed, c.env_offset, c.kind, goals if isinstance(goals, str) else tuple(goals))


# ------------------------------------------------------------------------------------------ counting what the states hold
def _situations_potential(ctx, st, e):
    from overcooked_ai_amd.potential import py_set_order

    found = set()
    who, pots = _players(ctx, st, e), _pot_view(ctx, st, e)
    cost = lambda p, k: ctx.c(who[p][0], who[p][1], ctx.pots[k])  # noqa: E731
    partial = [k for k, p in enumerate(pots) if p[0] in (1, 2)]
    holders = [(p, w[2]) for p, w in enumerate(who) if w[2] in (1, 2)]
    missing = lambda k, ing: ctx.opt[pots[k][1]][ing - 1]  # noqa: E731
    if len(partial) >= 2 and len(holders) == 1:
        h, ing = holders[0]
        ins = sorted(partial, key=lambda k: (pots[k][0], k))
        order = [ctx.pots.index(y * ctx.W + x) for (x, y) in py_set_order([(ctx.pots[k] % ctx.W, ctx.pots[k] // ctx.W) for k in ins])]
        sv = lambda k: ctx.sort_value[pots[k][1][0] + 4 * pots[k][1][1]]  # noqa: E731
        top = max(sv(k) for k in partial)
        group = [k for k in order if sv(k) == top]
        if len(group) >= 2 and all(missing(k, ing) > 0 for k in group[:2]) and \
                min(cost(h, group[0]), ctx.steps[ing]) != min(cost(h, group[1]), ctx.steps[ing]):
            found.add("set_order_matters")
            if len(partial) in (3, 4):
                found.add("three_or_four_partial")
            if len(partial) >= 5:
                found.add("set_resize")
            if len(partial) == 8:
                found.add("set_resize_all_eight")
        if len(pots) == 2 and pots[0][0] == 2 and pots[1][0] == 1 and all(missing(k, ing) > 0 for k in (0, 1)):
            found.add("set_order_two_then_one")
    if len(pots) == 2 and pots[0][0] == 2 and pots[1][0] == 1 and (pots[0][1], pots[1][1]) in ctx.tie_pairs and \
            any(w[2] == 0 for w in who) and len(set(_cook_dists(ctx, st, e, [w[:2] for w in who]))) == 2:
        found.add("set_order_bit1_tie")
    ni = [k for cls in (COOKING, READY) for k, p in enumerate(pots) if p[0] == cls]
    dish = [p for p, w in enumerate(who) if w[2] == 3]
    if len(pots) >= 2 and pots[0][0] == READY and pots[1][0] == COOKING and dish:
        found.add("ready_before_cooking")
    if len(dish) == 2 and len(ni) >= 2:
        found.add("two_dishes_two_soups")
        if _same_soup(ctx, st, e, [w[:2] for w in who]):
            found.add("two_dishes_same_soup")
    if ni and any(all(cost(p, k) == INF for k in ni) for p in dish):
        found.add("dish_unreachable")
    soup = [p for p, w in enumerate(who) if w[2] & 0x80]
    if soup:
        found.add("soup_in_hand")
        if any(not ctx.reach_serve[who[p][0]] for p in soup):
            found.add("soup_unservable")
    if any(p[0] == 3 for p in pots):
        found.add("full_idle_free_hand" if any(w[2] == 0 for w in who) else "full_idle_no_free_hand")
    if not partial and holders:
        empty = [k for k, p in enumerate(pots) if p[0] == EMPTY]
        if not empty:
            found.add("leftover_no_empty_pot")
        if sorted(i for _, i in holders) == [1, 2] and any(all(cost(p, k) != INF for p in range(2)) for k in empty):
            found.add("leftover_both_kinds")
    for p in pots:
        if p[0] == COOKING:
            found.add("long_cook" if p[2] > ctx.max_pick else "short_cook")
    if any(ctx.opt[pots[k][1]][0] > 0 and ctx.opt[pots[k][1]][1] > 0 for k in partial):
        found.add("mixed_completion")
    return found


def _situations_featurize(ctx, st, e, num_pots):
    found = set()
    who, pots = _players(ctx, st, e), _pot_view(ctx, st, e)
    for p, w in enumerate(who):
        for kind, code in KINDS:
            if w[2] == code or (code == 0x80 and w[2] & 0x80):
                found.add("held_%s_p%d" % (kind, p))
    rec = ctx.walk[4 * int(ctx.fidx[who[0][0]]) + who[0][1]]
    ranked = rec[16:32].view(np.uint32)
    for r in range(1, min(num_pots, 4) + 1):
        if ranked[r - 1] == 0xFFFFFFFF:
            found.add("pot%d_absent" % r)
        else:
            found.add("pot%d_%s" % (r, POT_CLASSES[pots[ctx.pots.index(int(ranked[r - 1]) & 0x7F)][0]]))
    if not ctx.goals_on:
        return found
    objects = [(c, int(st[1 + (c >> 4), e, c & 15])) for c in ctx.counters if st[1 + (c >> 4), e, c & 15]]
    for p, w in enumerate(who):
        cc = {c: _counter_cost(ctx, w, c) for c, _ in objects}
        for kind in (1, 2, 3):
            d = _dispenser_cost(ctx, w, kind)
            mine = [cc[c] for c, o in objects if o == kind]
            if w[2] != kind and d != 255 and mine and min(mine) < d:
                found.add("counter_beats_dispenser")
            if w[2] != kind and d != 255 and mine and min(mine) == d:
                found.add("counter_ties_dispenser")
        for c, o in objects:
            if o & 0x80 and cc[c] != 255:
                found.add("counter_soup")
                if o & 7:
                    found.add("counter_soup_tomato")
            if cc[c] == 255:
                found.add("counter_unreachable")
        n_goal = int(ctx.walk[4 * int(ctx.fidx[w[0]]) + w[1]][32])
        first = int(ctx.walk[4 * int(ctx.fidx[w[0]]) + w[1]][33])
        if n_goal and st[1 + (first >> 4), e, first & 15]:
            found.add("nearest_counter_taken")
    return found


def situations_of_states(table, lid, st, kind, goals="none", num_pots=2):
    """[set of situation names] per env, from the states and the host planner alone."""
    out = []
    for e in range(st.shape[1]):
        ctx = _ctx(table.specs[0 if lid is None else int(lid[e])], goals)
        out.append(_situations_potential(ctx, st, e) if kind == "potential" else _situations_featurize(ctx, st, e, num_pots))
    return out


def census_of(per_env):
    """{situation: (envs in which it holds, the fewest in any whole GROUP of envs)}"""
    names = sorted(set().union(*per_env)) if per_env else []
    n = len(per_env)
    out = {}
    for name in names:
        hit = np.array([name in s for s in per_env])
        whole = hit[:n - n % GROUP].reshape(-1, GROUP).sum(axis=1) if n >= GROUP else np.zeros((0,), int)
        out[name] = (int(hit.sum()), int(whole.min()) if len(whole) else 0)
    return out


@functools.lru_cache(maxsize=None)
def _census(cid):
    c = next(x for x in CASES if x.id == cid)
    goals = counter_goals_of(c) if c.kind == "featurize" else "none"
    return census_of(situations_of_states(table_of(c.table), layout_ids(c), states_of(c), c.kind, goals, c.num_pots or 0))


def census(c):
    return _census(c.id)


# ------------------------------------------------------------------------------------------ the planner's and the oracle's answers
def batch_of(c):
    """The OcBatch of the case's call with stand-in pointers: dispatch.batch_for's, its hints cleared where they are withheld."""
    from overcooked_ai_amd import dispatch

    b = dispatch.batch_for(table_of(c.table), c.n_envs)
    if not c.hints:
        b.max_pots = b.batch_flags = b.max_free_cells = 0
    return b


def plan_of_case(c):
    """oc_potential_plan's / oc_featurize_plan's answer for the call the case makes."""
    import ctypes

    from overcooked_ai_amd import _lib

    b, out = batch_of(c), ctypes.create_string_buffer(320)
    if c.kind == "potential":
        _lib.check(_lib.load().oc_potential_plan(ctypes.byref(b), out, len(out)), "oc_potential_plan")
    else:
        _lib.check(_lib.load().oc_featurize_plan(ctypes.byref(b), c.num_pots, out, len(out)), "oc_featurize_plan")
    return out.value.decode()


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedEnv the case runs on (layouts, n_envs and device aside)."""
    return dict(layout_id=layout_ids(c), seed=c.seed, env_offset=c.env_offset, withhold_hints=not c.hints)


@functools.lru_cache(maxsize=None)
def _oracle(table_name):
    return new_oracle(table_of(table_name).specs)


@functools.lru_cache(maxsize=None)
def _oracle_run(cid, gamma):
    from oracle import oracle as O
    from overcooked_ai_amd.potential import potential_params

    c = next(x for x in CASES if x.id == cid)
    table, orc = table_of(c.table), _oracle(c.table)
    if c.kind == "potential":
        out = O.potential(orc, states_of(c), [potential_params(s, gamma) for s in table.specs], layout_id=layout_ids(c))
    else:
        out = O.featurize(orc, states_of(c), counter_goals=counter_goals_of(c), num_pots=c.num_pots, layout_id=layout_ids(c))
    out.setflags(write=False)
    return out


def oracle_run(c, gamma=None):
    """The C oracle's answer, read-only, computed once: float64 [n_envs] phi at `gamma` (a potential case), or float32 [n_envs, 2,
    2 * (num_pots * 10 + 26) + 4] features."""
    return _oracle_run(c.id, None if c.kind == "featurize" else float(gamma))
