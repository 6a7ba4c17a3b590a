// mcts.h -- one wavefront advances one game: select / expand / backup, prior
// quantisation with Dirichlet noise, move choice, re-rooting and the hand-over
// between the two players' trees.
//
// Semantics follow the reference line by line (file:line cited at each
// function); the data layout does not (search_tree.h).  All floating-point
// expressions keep the reference's mixed float/double evaluation order
// (SURVEY 7 "hard parts" 1): this file must be compiled with
// -ffp-contract=off and correctly rounded fp32 division.
//
// The search in layers, each a header that includes the ones below it and calls only downward:
//   search_state.h  CoTree, CoWave, the phase stamps and the step's budget clock
//   search_tree.h   the tree's data layout (slot, node block); nodes and requests
//   search_eval.h   receiveEval: priors with Dirichlet noise, backups; propagateTerminal
//   search_puct.h   the PUCT arithmetic of one edge, the root copy
//   search_one.h    co_search: one simulation, the reference's way
//   search_group.h  co_search_rows: up to four simulations selected together
//   search_iter.h   co_mc_do_iteration: one player's share of a step
//   search_move.h   re-rooting, move choice, the opponent's move, text logs, analysis finish
//   search_step.h   co_game_step and the wavefront's step: gate, cache, budget, set-up, tail
#pragma once
#ifndef CO_EMU
#pragma clang fp contract(off)
#endif
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_puct.h"
#include "search_one.h"
#include "search_group.h"
#include "search_iter.h"
#include "search_move.h"
#include "search_step.h"
