"""Hand-overs between the autograd nodes of one stage-3 evaluation for the turn-around riders (include/humor_amd.h, "Turn-around riders").

Around the one-launch roll-out of up to 32 sequences three short launches depend on nothing their neighbours write; the node next to the
roll-out runs them as extra blocks of a launch it makes anyway and the roll-out entry point is told so with flag bits:

  Stage3Head.forward    ha_fit_pre_forward clears the exchange words of the persistent forward         -> HA_ROLL_CLEARED
  Stage3Body.backward   ha_rollout_post_backward lays g_prior_mu / g_prior_var out for the prior's
                        adjoint and clears the exchange words of the persistent adjoint                 -> HA_ROLL_LAID_OUT | HA_ROLL_CLEARED
  Stage3Head.backward   ha_fit_pre_backward adds up the dL/dz partials the persistent adjoint left      <- HA_ROLL_DEFER_DZ

The nodes of an evaluation share one `box` (a dict made per evaluation by MotionOptimizer._stage3_objective_nodes, handed to the roll-out node
through HumorModel.roll_out(turn=box) and to the stage-3 nodes as cfg['turn']).  Whether a part rides is the library's decision
(ha_humor_rollout_turn_tasks: the B <= 32 persistent kernels, "turn_merge"); every claim a node makes to the roll-out entry point is checked
there against the mark the riding launch left, so a hand-over that did not happen is an error, never a wrong gradient."""
import ctypes as C

from . import _lib

# device -> (data_ptr of the roll-out's prior_mu output, box): the evaluation whose loss node is asked to hand its prior gradients over
_EXPECT = {}


def new_box(handle, S, z_leaf=None):
    """z_leaf: the latent sequence when the tensor the roll-out reads IS the optimisation variable (no slice, no shard) -- only then nothing
    reads the roll-out's g_z between the roll-out's backward and the head's, and the dL/dz reduction may be deferred to the head."""
    return {'handle': handle, 'S': int(S), 'z_leaf': z_leaf}


def tasks(box, lib, B, S, stash, adjoint):
    t = _lib.TurnTasks()
    lib.call('ha_humor_rollout_turn_tasks', box['handle'].ptr, B, S, _lib.ptr(stash), 1 if adjoint else 0, C.byref(t))
    return t


def expect_prior_grads(box, pm):
    _EXPECT[pm.device] = (pm.data_ptr(), box)


def offer_prior_grads(device, key, g_mu, g_var):
    """Called by the loss node's backward with the gradients of its prior_mu / prior_var inputs (key: data_ptr of prior_mu)."""
    e = _EXPECT.get(device)
    if e is not None and e[0] == key:
        del _EXPECT[device]
        e[1]['g_prior'] = (g_mu, g_var)
